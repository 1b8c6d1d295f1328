"""CPU tests of the recompute chain's saved state (``fused_chain.ChainState``, ``take_set_saved``): the order in which
its tensors pass through ``ctx.save_for_backward`` is ``CHAIN_SAVED``, and the backward's once-only guard."""
from types import SimpleNamespace

import pytest
import torch

from deepviewagg_amd import fused_chain as FC

ORDER = ("vp", "tiles", "n_tiles", "wops", "t_add", "zstar", "arg", "mom", "bn1", "bn2", "bn5", "bn6")


def _state():
    tensors = {name: torch.full((2,), float(i)) for i, name in enumerate(ORDER)}
    extras = dict(W1=torch.full((3,), 100.0), bs=torch.full((3,), 101.0), gw=torch.full((3,), 102.0),
                  gb=torch.full((3,), 103.0), G=4, training=True, set_saved=("set", "branch"))
    return FC.ChainState(**tensors, **extras), tensors, extras


def test_saved_follows_chain_saved():
    assert FC.CHAIN_SAVED == ORDER          # tests/test_gpu_chain.py and two more index ctx.saved_tensors by these positions
    state, tensors, _ = _state()
    saved = state.saved()
    assert len(saved) == 12
    for i, name in enumerate(FC.CHAIN_SAVED):
        assert saved[i] is tensors[name] and getattr(state, name) is tensors[name]
        assert float(saved[i][0]) == i      # twelve distinct tensors: no two names share one


def test_restore_inverts_saved():
    state, tensors, extras = _state()
    back = FC.ChainState.restore(list(state.saved()), W1=extras["W1"], G=32, training=False)
    for a, b in zip(back.saved(), state.saved(), strict=True):
        assert a is b
    assert back.W1 is extras["W1"] and back.G == 32 and back.training is False
    assert back.bs is None and back.gw is None and back.gb is None and back.set_saved is None     # forward only
    assert state.bs is extras["bs"] and state.gw is extras["gw"] and state.gb is extras["gb"]
    assert state.set_saved == ("set", "branch") and state.G == 4 and state.training is True
    with pytest.raises(TypeError):
        FC.ChainState.restore(list(state.saved())[:-1], W1=extras["W1"], G=4, training=True)


@pytest.mark.parametrize("say_released,text", [(False, "same graph (retain_graph"),
                                               (True, "same graph: its per-step workspaces are released after")])
def test_take_set_saved_hands_out_once(say_released, text):
    ctx = SimpleNamespace(set_saved=("pooled", "sops"))
    assert FC.take_set_saved(ctx, say_released) == ("pooled", "sops")
    assert ctx.set_saved is None
    with pytest.raises(RuntimeError, match="ran twice") as err:
        FC.take_set_saved(ctx, say_released)
    assert text in str(err.value) and "retain_graph is not supported on this path" in str(err.value)
