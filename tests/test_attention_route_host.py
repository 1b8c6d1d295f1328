"""CPU tests of ``ops.attention_bwd_route``: which backward of ``view_gather_attention`` runs, one named row per boundary
of the dispatch, the expected route written out."""
import pytest
import torch

from deepviewagg_amd import _lib, ops

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
MAX = _lib.BUFFER_BYTES_MAX


def _first_at(limit, step):
    """The smallest count whose ``count * step`` bytes reach ``limit`` (``count - 1`` is the last one below it)."""
    return -(-limit // step)


# the base case: fp32 rows [16, 32], four score groups, 91 views of 9 points, aligned, rows gradient wanted
BASE = dict(rows_dtype=F32, gout_dtype=F32, out_dtype=F32, C=32, G=4, V=91, R=16, N=9, need_rows=True, aligned16=True)
B16 = dict(rows_dtype=BF16, gout_dtype=BF16, out_dtype=BF16)
H16 = dict(rows_dtype=F16, gout_dtype=F16, out_dtype=F16)
NO_SWITCH = {}

# name: (changes to BASE, module switches, (kernel, rows_grad, records))
CASES = {
    "f32_c32_g4": ({}, NO_SWITCH, ("lean_f32", "plan", False)),
    "f32_c256_g4": (dict(C=256), NO_SWITCH, ("lean_f32", "plan", False)),
    "f32_g2_team_records_lpr8": (dict(G=2), NO_SWITCH, ("team", "plan", True)),
    "f32_c20_generic": (dict(C=20), NO_SWITCH, ("team", "plan", False)),
    "f32_c512": (dict(C=512), NO_SWITCH, ("team", "plan", False)),
    "f32_gout_bf16": (dict(gout_dtype=BF16), NO_SWITCH, ("team", "plan", True)),
    "f32_no_views": (dict(V=0), NO_SWITCH, ("team", "plan", True)),
    "f32_records_below_limit": (dict(V=_first_at(MAX, 32) - 1), NO_SWITCH, ("lean_f32", "plan", False)),
    "f32_records_at_limit": (dict(V=_first_at(MAX, 32)), NO_SWITCH, ("team", "plan", True)),
    "f32_rows_below_limit": (dict(R=_first_at(MAX, 32 * 4) - 1), NO_SWITCH, ("lean_f32", "plan", False)),
    "f32_rows_at_limit": (dict(R=_first_at(MAX, 32 * 4)), NO_SWITCH, ("team", "plan", True)),
    "f32_points_at_limit": (dict(N=_first_at(MAX, 32 * 4)), NO_SWITCH, ("team", "plan", True)),
    "bf16_g1": (dict(B16, G=1), NO_SWITCH, ("lean_16", "plan", False)),
    "bf16_g2": (dict(B16, G=2), NO_SWITCH, ("lean_16", "plan", False)),
    "bf16_g4": (dict(B16, G=4), NO_SWITCH, ("lean_16", "plan", False)),
    "bf16_c64_g8": (dict(B16, C=64, G=8), NO_SWITCH, ("team", "plan", True)),
    "bf16_c32_g8": (dict(B16, G=8), NO_SWITCH, ("team", "plan", False)),
    "fp16_g1": (dict(H16, G=1), NO_SWITCH, ("lean_16", "plan", False)),
    "fp16_g2": (dict(H16, G=2), NO_SWITCH, ("lean_16", "plan", False)),
    "fp16_g4": (dict(H16, G=4), NO_SWITCH, ("lean_16", "plan", False)),
    "fp16_c64_g8": (dict(H16, C=64, G=8), NO_SWITCH, ("team", "plan", True)),
    "bf16_c512": (dict(B16, C=512), NO_SWITCH, ("lean_16", "plan", False)),
    "bf16_out_f32": (dict(B16, out_dtype=F32), NO_SWITCH, ("team", "plan", True)),
    "bf16_gout_f32": (dict(B16, gout_dtype=F32), NO_SWITCH, ("team", "plan", True)),
    "bf16_no_views": (dict(B16, V=0), NO_SWITCH, ("team", "plan", True)),
    "bf16_records_below_limit": (dict(B16, V=MAX // 16 - 1), NO_SWITCH, ("lean_16", "plan", False)),
    "bf16_records_at_limit": (dict(B16, V=MAX // 16), NO_SWITCH, ("team", "plan", True)),      # V * 16 == MAX exactly
    "bf16_rows_below_limit": (dict(B16, N=_first_at(MAX, 32 * 2) - 1), NO_SWITCH, ("lean_16", "plan", False)),
    "bf16_rows_at_limit": (dict(B16, N=_first_at(MAX, 32 * 2)), NO_SWITCH, ("team", "plan", True)),
    "bf16_map_rows_at_limit": (dict(B16, R=_first_at(MAX, 32 * 2)), NO_SWITCH, ("team", "plan", True)),
    "f32_no_rows_gradient": (dict(need_rows=False), NO_SWITCH, ("team", "none", False)),
    "bf16_no_rows_gradient": (dict(B16, need_rows=False), NO_SWITCH, ("team", "none", False)),
    "f32_atomics": ({}, dict(ROWS_GRAD_ALGO=1), ("team", "atomics", False)),
    "bf16_atomics": (B16, dict(ROWS_GRAD_ALGO=1), ("team", "atomics", False)),
    "f32_generic_algo": ({}, dict(ATTENTION_ALGO=1), ("team", "plan", False)),
    "bf16_generic_algo": (B16, dict(ATTENTION_ALGO=1), ("team", "plan", False)),
    "f32_team_algo_stays_lean": ({}, dict(ATTENTION_ALGO=2), ("lean_f32", "plan", False)),
    "f32_lean_off": ({}, dict(LEAN_ATTENTION_BWD=False), ("team", "plan", True)),
    "bf16_lean_off": (B16, dict(LEAN_ATTENTION_BWD=False), ("team", "plan", True)),
    "f32_g2_unaligned": (dict(G=2, aligned16=False), NO_SWITCH, ("team", "plan", False)),
    "f32_lean_ignores_alignment": (dict(aligned16=False), NO_SWITCH, ("lean_f32", "plan", False)),
}


def test_the_limit_rows_straddle_the_limit():
    """The table's limit rows are what they are named: MAX is a multiple of 16 and of no larger power of two."""
    assert MAX == (1 << 32) - 16 and (MAX // 16) * 16 == MAX
    for step in (32, 32 * 4, 32 * 2):
        n = _first_at(MAX, step)
        assert (n - 1) * step < MAX <= n * step


@pytest.mark.parametrize("name", list(CASES))
def test_route(name, monkeypatch):
    changes, switches, expect = CASES[name]
    for key, value in switches.items():
        monkeypatch.setattr(ops, key, value)
    route = ops.attention_bwd_route(**dict(BASE, **changes))
    assert tuple(route) == expect
    assert (route.kernel, route.rows_grad, route.records) == expect
    assert type(route.records) is bool


def test_switches_are_read_at_call_time(monkeypatch):
    args = dict(BASE)
    assert ops.attention_bwd_route(**args).kernel == "lean_f32"
    monkeypatch.setattr(ops, "LEAN_ATTENTION_BWD", False)
    assert ops.attention_bwd_route(**args).kernel == "team"
    monkeypatch.undo()
    assert ops.attention_bwd_route(**args).kernel == "lean_f32"


def test_fits_buffer():
    assert _lib.fits_buffer() and _lib.fits_buffer(0, MAX - 1)
    assert not _lib.fits_buffer(MAX) and not _lib.fits_buffer(0, MAX - 1, MAX + 5)
