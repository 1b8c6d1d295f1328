"""No GPU: the seven wrappers of the mapping ops give one verdict for one fault.  Shapes come first (``ValueError``),
then what the kernels do not take (``DvaError`` with ``code == -2``), then the device (``DvaError`` without a code), and
every message of an argument check starts with the op's name.  A fault is tried on every op that takes the tensor it
sits in: ``MappingCoverage`` takes ``pointers`` and ``images`` only, the image stats and the two rolls no ``pointers``.
Also ``_lib.unless_unsupported``, the callers' one guard."""
import pytest
import torch

from image_pick_ref import mapping_from_views


def mapping():
    """2 points, 2 views, 3 atoms, 4 feature channels."""
    m = dict(zip(("pointers", "images", "atom_ptr", "pixels"),
                 (torch.from_numpy(a) for a in mapping_from_views(2, [(0, 0, [1, 2]), (1, 1, [3])]))))
    assert [m[k].shape[0] for k in ("pointers", "images", "atom_ptr", "pixels")] == [3, 2, 3, 3]
    m["features"] = torch.zeros(2, 4)
    return m


def vector(n):
    return torch.zeros(n, dtype=torch.int64)


MAPPING = ("pointers", "images", "atom_ptr", "pixels", "features")
VIEWS = ("images", "atom_ptr", "pixels")
# op -> (the call on a mapping dict, the tensors of the mapping it takes)
WRAPPERS = {
    "merge_mapping": (lambda ops, m: ops.merge_mapping(*[m[k] for k in MAPPING], vector(2)), MAPPING),
    "select_mapping": (lambda ops, m: ops.select_mapping(*[m[k] for k in MAPPING], point_idx=vector(1)), MAPPING),
    "mapping_image_stats": (lambda ops, m: ops.mapping_image_stats(*[m[k] for k in VIEWS], 2), VIEWS),
    "mapping_center_rollings": (lambda ops, m: ops.mapping_center_rollings(*[m[k] for k in VIEWS], 2, 64), VIEWS),
    "roll_mapping_pixels": (lambda ops, m: ops.roll_mapping_pixels(*[m[k] for k in VIEWS], vector(2), 64), VIEWS),
    "MappingCoverage": (lambda ops, m: ops.MappingCoverage([(m["pointers"], m["images"], 2)], 2),
                        ("pointers", "images")),
    "collate_mapping": (lambda ops, m: ops.collate_mapping([tuple(m[k] for k in MAPPING)]), MAPPING),
}
UNSUPPORTED = -2
# fault -> (the tensor, what happens to it, the verdict)
FAULTS = {
    "int32_pointers": ("pointers", lambda t: t.int(), UNSUPPORTED),
    "int32_images": ("images", lambda t: t.int(), UNSUPPORTED),
    "int32_atom_ptr": ("atom_ptr", lambda t: t.int(), UNSUPPORTED),
    "int32_pixels": ("pixels", lambda t: t.int(), UNSUPPORTED),
    "images_2d": ("images", lambda t: t.view(-1, 1), ValueError),
    "pixels_p3": ("pixels", lambda t: torch.cat([t, t[:, :1]], dim=1), ValueError),
    "atom_ptr_short": ("atom_ptr", lambda t: t[:-1], ValueError),
}
CASES = [(op, fault) for op, (_, takes) in WRAPPERS.items() for fault, (name, _, _) in FAULTS.items() if name in takes]


def refusal(op, m):
    """The exception ``ops.<op>`` raises for the mapping ``m``."""
    from deepviewagg_amd import ops
    from deepviewagg_amd._lib import DvaError
    with pytest.raises((ValueError, DvaError)) as err:
        WRAPPERS[op][0](ops, m)
    return err.value


@pytest.mark.parametrize("op,fault", CASES, ids=[f"{op}-{fault}" for op, fault in CASES])
def test_one_fault_one_verdict(op, fault):
    from deepviewagg_amd._lib import DvaError
    name, spoil, verdict = FAULTS[fault]
    m = mapping()
    m[name] = spoil(m[name])
    e = refusal(op, m)
    if verdict is ValueError:
        assert type(e) is ValueError
    else:
        assert type(e) is DvaError and e.code == verdict
    assert str(e).startswith(f"ops.{op}:") and name in str(e)


def test_every_fault_is_tried_on_every_op_that_takes_its_tensor():
    assert {op for op, _ in CASES} == set(WRAPPERS) and len(WRAPPERS) == 7
    for fault in ("int32_images", "images_2d"):
        assert sum(f == fault for _, f in CASES) == 7
    for fault in ("int32_pixels", "pixels_p3", "atom_ptr_short"):
        assert sum(f == fault for _, f in CASES) == 6      # all but MappingCoverage


@pytest.mark.parametrize("op", WRAPPERS)
def test_correct_host_tensors_reach_the_device_refusal(op):
    from deepviewagg_amd._lib import DvaError
    e = refusal(op, mapping())
    assert type(e) is DvaError and e.code is None


@pytest.mark.parametrize("op,code", [("select_mapping", UNSUPPORTED), ("collate_mapping", UNSUPPORTED),
                                     ("merge_mapping", None)])
def test_fp64_features(op, code):
    """Selection and collation copy the features as bits and take fp32 only; the merge casts, so its argument checks
    pass and the device refusal is what is left."""
    from deepviewagg_amd._lib import DvaError
    m = mapping()
    m["features"] = m["features"].double()
    e = refusal(op, m)
    assert type(e) is DvaError and e.code == code
    if code is not None:
        assert str(e).startswith(f"ops.{op}:") and "features" in str(e)


def test_a_wrong_shape_wins_over_a_wrong_dtype_and_both_over_the_device():
    from deepviewagg_amd._lib import DvaError
    for op in WRAPPERS:
        m = mapping()
        m["pointers"], m["images"] = m["pointers"].int(), m["images"].int().view(-1, 1)
        assert type(refusal(op, m)) is ValueError
        m["images"] = m["images"].view(-1)
        e = refusal(op, m)
        assert type(e) is DvaError and e.code == UNSUPPORTED


def test_unless_unsupported():
    from deepviewagg_amd import _lib

    def raising(exc):
        raise exc
    assert _lib.DVA_ERR_UNSUPPORTED == -2 and _lib.DVA_ERR_UNSUPPORTED in _lib._ERRORS
    assert _lib.unless_unsupported(raising, _lib.DvaError("declined", code=-2)) is None
    for exc in (_lib.DvaError("bad argument", code=-1), _lib.DvaError("no device"), ValueError("shape")):
        with pytest.raises(type(exc)) as err:
            _lib.unless_unsupported(raising, exc)
        assert err.value is exc
    assert _lib.unless_unsupported(lambda a, b=0: (a, b), 1, b=2) == (1, 2)
