"""The address rule of ctrlora_amd/engine/packing.py, the part that needs no GPU: a derived pack (Conv3W's phase packs,
LinearW's GEGLU pack) that exists is refreshed IN PLACE by a weight load -- same tensor object, same address, the values a
freshly packed object holds -- and a pack that was never built stays unbuilt."""
import pytest
import torch

from tests.flags_common import netcfg
from oracle import arch

KINDS = ("up2", "t2", "up2d")


def _conv_weights(seed, O=128, I=128):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(O, I, 3, 3, generator=g) * (1.0 / (3 * I ** 0.5)), torch.randn(O, generator=g) * 0.1


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_conv3w_load_refreshes_built_phase_packs_in_place(dtype):
    from ctrlora_amd.engine.packing import Conv3W
    (W0, b0), (W1, b1) = _conv_weights(1), _conv_weights(2)
    cw = Conv3W(W0, b0, dtype, "cpu", True)
    assert cw._phase == {}                                        # the constructor's own load() builds nothing
    held = {k: cw.phase_weights(k) for k in KINDS}
    before = {k: (t.data_ptr(), t.shape, t.dtype, t.clone()) for k, t in held.items()}
    only_up2 = Conv3W(W0, b0, dtype, "cpu", True)
    only_up2.phase_weights("up2")
    cw.load(W1, b1)
    only_up2.load(W1, b1)
    fresh = Conv3W(W1, b1, dtype, "cpu", True)
    assert sorted(cw._phase) == sorted(KINDS)
    for k in KINDS:
        ptr, shape, dt, old = before[k]
        assert cw._phase[k] is held[k] and cw.phase_weights(k) is held[k]
        assert (held[k].data_ptr(), held[k].shape, held[k].dtype) == (ptr, shape, dt)
        assert torch.equal(held[k], fresh.phase_weights(k)), k
        assert not torch.equal(held[k], old), k                   # (the load did change the weights)
    assert list(only_up2._phase) == ["up2"]
    assert torch.equal(only_up2._phase["up2"], fresh.phase_weights("up2"))


def test_conv3w_made_trainable_drops_its_phase_packs_on_load():
    from ctrlora_amd.engine.packing import Conv3W, Trainable
    (W0, b0), (W1, b1) = _conv_weights(1), _conv_weights(2)
    cw = Conv3W(W0, b0, torch.float32, "cpu", True)
    cw.phase_weights("t2")
    cw.attach_trainable(Trainable("w", (128, 9 * 128)), Trainable("b", (128,)))
    cw.load(W1, b1)
    assert cw._phase == {}
    with pytest.raises(AssertionError, match="frozen convs only"):
        cw.phase_weights("t2")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_linearw_load_refreshes_the_geglu_pack_in_place(dtype):
    from ctrlora_amd.engine.packing import LinearW
    g = torch.Generator().manual_seed(3)
    W0, W1 = torch.randn(640, 64, generator=g), torch.randn(640, 64, generator=g)
    bias = torch.randn(640, generator=g)
    L = LinearW(W0, bias, dtype, "cpu", True)
    assert L.geglu_ok()
    Wg, bg, Bg = L.geglu_pack()
    assert Bg is None and L.geglu_pack()[0] is Wg                 # (no LoRA; a second call without a load is the same pack)
    ptrs, old = (Wg.data_ptr(), bg.data_ptr()), Wg.clone()
    L.load(W1, None)
    Wg1, bg1, Bg1 = L.geglu_pack()
    assert Wg1 is Wg and bg1 is bg and Bg1 is None
    assert (Wg.data_ptr(), bg.data_ptr()) == ptrs
    fWg, fbg, _ = LinearW(W1, bias, dtype, "cpu", True).geglu_pack()
    assert Wg.dtype == fWg.dtype and torch.equal(Wg, fWg) and torch.equal(bg, fbg)
    assert not torch.equal(Wg, old)


def test_geglu_pack_refuses_a_refresh_from_another_source():
    """Which weight feeds the pack (W or the folded Wm) is settled by the first build: a fold that appears afterwards would
    need new storage, so the refresh raises instead of reallocating."""
    from ctrlora_amd.engine.packing import LinearW
    g = torch.Generator().manual_seed(4)
    L = LinearW(torch.randn(640, 64, generator=g), None, torch.float32, "cpu", False)
    L.geglu_pack()
    L.Wm = L.W.clone()
    L.invalidate_geglu()
    with pytest.raises(RuntimeError, match="cannot be refreshed in place"):
        L.geglu_pack()


def _conv_layers(ex):
    """(state-dict name, Conv3W) of every plain conv layer of the encoder: block k of the executor is input_blocks.k."""
    from ctrlora_amd import hip
    from ctrlora_amd.engine.nets import _Conv
    out = []
    for k, layers in enumerate(list(ex.blocks) + [ex.mid]):
        for l in layers:
            if isinstance(l, _Conv):
                out.append((f"input_blocks.{k}.0" + (".op" if l.mode == hip.CONV_S2 else ""), l.cw))
    return out


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_reload_frozen_keeps_every_phase_pack_of_the_executor_in_place(dtype):
    from ctrlora_amd.engine import ControlNetE
    from ctrlora_amd.engine.packing import Conv3W
    cfg = arch.TINY
    shapes = arch.controlnet_shapes(cfg)
    ex = ControlNetE(arch.make_state(shapes, 1), netcfg(cfg), dtype, torch.device("cpu"), layout_only=True)
    convs = _conv_layers(ex)
    before = {(n, k): (t, t.data_ptr(), t.clone()) for n, cw in convs for k, t in cw._phase.items()}
    assert sorted(before) == sorted((f"input_blocks.{i}.0.op", "t2") for i in (3, 6, 9))      # the three Downsample convs
    new = arch.make_state(shapes, 2)
    ex._b.reload_frozen(new)
    after = {(n, k): t for n, cw in convs for k, t in cw._phase.items()}
    assert sorted(after) == sorted(before)
    for (n, k), (t, ptr, old) in before.items():
        assert after[(n, k)] is t and t.data_ptr() == ptr
        fresh = Conv3W(new[n + ".weight"], new[n + ".bias"], dtype, "cpu", True)
        assert torch.equal(t, fresh.phase_weights(k)), (n, k)
        assert not torch.equal(t, old), (n, k)
