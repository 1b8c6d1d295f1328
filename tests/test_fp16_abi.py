"""CPU test: the float16 storage type of the C ABI (DVA_F16).  The code agrees between dva.h and the ctypes binding,
the library reports the version that introduced it, and the dtype-taking chain entries validate their arguments
before any HIP call."""
import os
import re

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
