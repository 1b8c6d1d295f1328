"""CPU test: the float16 storage type of the C ABI (DVA_F16).  The code agrees between dva.h and the ctypes binding,
the library reports the version that introduced it, and the dtype-taking chain entries validate their arguments
before any HIP call."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT
from deepviewagg_amd import _lib


def test_f16_code_agrees_everywhere():
    text = open(os.path.join(ROOT, "include", "dva.h")).read()
    m = re.search(r"#define DVA_F16 (\d+)", text)
    assert m and int(m.group(1)) == 2
    assert _lib.DVA_F16 == 2
    assert _lib.dtype_code(torch.empty(1, dtype=torch.float16)) == 2
    assert _lib.dtype_code(torch.empty(1, dtype=torch.bfloat16)) == _lib.DVA_BF16


def test_version_has_f16():
    assert _lib.load().dva_version() >= 307


_BUF = ctypes.create_string_buffer(256)
_P = ctypes.addressof(_BUF)     # a non-null pointer: the host side of an entry never dereferences its device pointers
_BIG = 1 << 40                  # a workspace size that passes every size check
_DT = "dtype"                   # where the dtype code goes

# Every entry that picks its kernel through with_dtype / with_f32_bf16: sizes >= 1 and pointers non-null, so that nothing
# but the dtype code is left to refuse.
_DISPATCHED = {
    "dva_gather_nearest_fwd": (_P, _P, _P, 1, 1, 2, 2, 4, _DT, None),
    "dva_gather_nearest_bwd": (_P, _P, _P, 1, 1, 2, 2, 4, _DT, None),
    "dva_gather_bilinear_fwd": (_P, _P, _P, _P, 1, 1, 2, 2, 4, _DT, None),
    "dva_gather_bilinear_bwd": (_P, _P, _P, _P, 1, 1, 2, 2, 4, _DT, None),
    "dva_anchor_fixup": (_P, _P, _P, _P, _P, 1, 1, 2, 2, 4, _DT, None),
    "dva_segment_csr_fwd": (_P, _P, _P, _P, 1, 4, _DT, _lib.DVA_SUM, None),
    "dva_segment_csr_bwd": (_P, _P, _P, _P, 1, 4, _DT, _lib.DVA_MAX, None),
    "dva_gather_csr": (_P, _P, _P, 1, 4, _DT, None),
    "dva_rowbn_stats": (_P, _P, _P, 1, 4, _DT, None),
    "dva_rowbn_apply": (_P, _P, _P, 1, 4, 0.1, _DT, None),
    "dva_rowbn_bwd_stats": (_P, _P, _P, _P, 1, 4, 0.1, _DT, None),
    "dva_rowbn_bwd_apply": (_P, _P, _P, _P, _P, _P, 1, 4, 0.1, _DT, None),
    "dva_view_attention_fwd": (*[_P] * 9, 1, 1, 8, 2, 1, 1e-12, _DT, 0, None),
    "dva_view_attention_bwd": (*[_P] * 12, 1, 1, 8, 2, 1, _DT, 0, None),
    "dva_view_gather_attention_fwd": (*[_P] * 10, 1, 1, 8, 2, 1, 1e-12, _DT, 0, None),
    "dva_view_gather_attention_bwd": (*[_P] * 13, None, 0, 1, 1, 8, 2, 1, _DT, 0, None),
    "dva_view_attention_geometry": (64, 4, 1, 1, _DT, _P, _P),
    "dva_view_gather_rows_grad": (_P, _P, _P, _P, _P, _P, None, 0, _P, 1, 1, 8, 2, _DT, None),
    "dva_view_gather_rows_grad_rec16_to": (_P, _P, _P, _P, _P, _lib.DVA_F32, 1, 1, 8, 1, _DT, None),
    "dva_gather_rows_sum": (_P, _P, _P, _P, 0, _P, 1, 1, 8, _DT, None),
    "dva_anchor_rows_sum": (_P, _P, _P, _P, _P, 1, 1, 8, _DT, None),
    "dva_view_nll_fwd": (_P, _DT, _P, _P, 1, 4, _P, _P, _P, _BIG, None),
    "dva_view_nll_bwd": (_P, _DT, _P, _P, _P, _P, 1, 4, _P, None),
    "dva_seg_logsoftmax_nll_fwd": (_P, _DT, _P, _P, -1, 1, 4, _P, _P, _P, _P, _BIG, None),
    "dva_seg_logsoftmax_nll_bwd": (_P, _P, _P, _P, _P, _P, -1, 1, 4, _P, _DT, None),
    "dva_confusion_counts": (_P, _DT, _P, -1, 1, 4, _P, _P, None),
    "dva_vote_add": (_P, _P, 1, 4, _P, _P, _DT, 1, _P, _BIG, _P, None),
    "dva_concat_cast_fwd": (_P, _P, _P, 4, 4, 4, _DT, None),
    "dva_concat_cast_bwd": (_P, _P, _P, 4, 4, 4, _DT, None),
}
# What an unknown code answers where it is not DVA_ERR_INVALID: the 16-byte records of rows_grad_rec16_to go with 2-byte
# rows, and the entry answers every other dtype, known or not, as unsupported (its out_dtype is checked as the others are)
_UNKNOWN_ANSWER = {"dva_view_gather_rows_grad_rec16_to": -2}
# fp32 / bf16 only: DVA_F16 is a known code without kernels
_NO_F16 = ("dva_anchor_fixup", "dva_anchor_rows_sum", "dva_concat_cast_fwd", "dva_concat_cast_bwd")


def _call(lib, name, dtype):
    return getattr(lib, name)(*[dtype if a is _DT else a for a in _DISPATCHED[name]])


@pytest.mark.parametrize("name", sorted(_DISPATCHED))
@pytest.mark.parametrize("code", [3, -1])
def test_unknown_dtype_is_invalid_before_any_launch(name, code):
    assert _call(_lib.load(), name, code) == _UNKNOWN_ANSWER.get(name, -1)


@pytest.mark.parametrize("code", [3, -1])
def test_unknown_out_dtype_of_rec16_rows_is_invalid(code):
    args = list(_DISPATCHED["dva_view_gather_rows_grad_rec16_to"])
    args[5], args[10] = code, _lib.DVA_BF16
    assert _lib.load().dva_view_gather_rows_grad_rec16_to(*args) == -1


@pytest.mark.parametrize("name", _NO_F16)
def test_f32_bf16_entries_answer_f16_unsupported(name):
    assert _call(_lib.load(), name, _lib.DVA_F16) == -2


def test_new_entries_validate_without_gpu():
    lib = _lib.load()
    none18 = [None] * 18
    none14 = [None] * 14
    # null pointers with views to pool: DVA_ERR_INVALID
    assert lib.dva_chain_attn_fwd_dt(*none18, 4, 8, 8, 64, 4, 1, 1e-12, _lib.DVA_F16, None) == -1
    assert lib.dva_chain_attn_bwd_dt(*none14, 4, 8, 8, 64, 4, 1, 1e-12, _lib.DVA_F16, None) == -1
    # an unknown dtype code: DVA_ERR_INVALID (before the pointers are looked at)
    assert lib.dva_chain_attn_fwd_dt(*none18, 4, 8, 8, 64, 4, 1, 1e-12, 3, None) == -1
    assert lib.dva_chain_attn_bwd_dt(*none14, 4, 8, 8, 64, 4, 1, 1e-12, 3, None) == -1
    # entries outside the fp16 list refuse it as unsupported, not as a bad argument
    assert lib.dva_sparse_conv_workspace_bytes(27, 16, 16, _lib.DVA_F16) == -2
    assert lib.dva_concat_cast_fwd(None, None, None, 4, 4, 4, _lib.DVA_F16, None) == -2
    assert lib.dva_deepset_fwd_layer(None, None, None, None, None, None, None, 0, _lib.DVA_F16, None) == -2
