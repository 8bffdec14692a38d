"""The address rule of ctrlora_amd/engine/packing.py on the GPU (run with -m gpu on an MI355X): a launch captured into a graph
keeps the pointers it was given, so a weight load has to rewrite every packed tensor -- the derived packs included -- where it
lies.  (1) One captured phase-form product per kind of Conv3W.phase_weights replays the weights loaded after the capture.
(2) No packed tensor of the fine-tuning model's control executor moves across control_model.load_state_dict().

The bit-equality in (1) is derived, not measured: the replay and the eager call on a freshly packed conv run the same kernel in
the same configuration on equal operands, and where the launcher splits K it sums the slabs through the workspace in a fixed
order (header of csrc/gemm.hip)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from ctrlora_amd import hip
    hip.lib()


def _conv_weights(seed, O=128, I=128):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(O, I, 3, 3, generator=g) * (1.0 / (3 * I ** 0.5)), torch.randn(O, generator=g) * 0.1


def _phase_call(kind):
    """(input rows, output rows, launch(cw, x, out)): the launches of blocks.conv3_fwd / conv3_bwd_data at batch 2, 128 -> 128
    channels, made with hip.gemm directly so that no launch rule is involved."""
    from ctrlora_amd import hip
    if kind == "up2":
        return 128, 512, lambda cw, x, out: hip.gemm(x, cw.phase_weights("up2"), out, bias=cw.bias, mode=hip.CONV_UP2P,
                                                     conv=(2, 8, 8, 16, 16), k1=128, N=128)
    if kind == "t2":
        return 128, 512, lambda cw, x, out: hip.gemm(x, cw.phase_weights("t2"), out, mode=hip.CONV_T2P,
                                                     conv=(2, 8, 8, 16, 16), k1=cw.Op, N=cw.Ip)
    return 512, 128, lambda cw, x, out: hip.gemm(x, cw.phase_weights("up2d"), out, mode=hip.CONV_S2K4,
                                                 conv=(2, 16, 16, 8, 8), k1=cw.Op, N=cw.Ip)


@pytest.mark.parametrize("kind", ["up2", "t2", "up2d"])
def test_captured_phase_product_replays_the_weights_loaded_after_the_capture(kind):
    _need_gpu()
    from ctrlora_amd.engine.packing import Conv3W
    (W0, b0), (W1, b1) = _conv_weights(11), _conv_weights(12)
    rows_in, rows_out, launch = _phase_call(kind)
    cw = Conv3W(W0, b0, BF, "cuda", True)
    assert (cw.Ip, cw.Op) == (128, 128)
    x = torch.randn(rows_in, 128, generator=torch.Generator().manual_seed(13)).to(BF).cuda().contiguous()
    out = torch.empty(rows_out, 128, dtype=BF, device="cuda")
    launch(cw, x, out)                                    # eager: the pack exists, the workspace is registered
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch(cw, x, out)
    graph.replay()
    torch.cuda.synchronize()
    y0 = out.clone()
    cw.load(W1, b1)
    graph.replay()
    torch.cuda.synchronize()
    y1 = out.clone()
    del graph
    y_ref = torch.empty_like(out)
    launch(Conv3W(W1, b1, BF, "cuda", True), x, y_ref)
    torch.cuda.synchronize()
    assert torch.equal(y1, y_ref)
    assert not torch.equal(y1, y0)


def _packed_tensors(ex):
    """name -> tensor for every packed tensor of a ControlNetE, the flat master / gradient buffers included."""
    from ctrlora_amd.engine.nets import _Conv, _Res
    out = {"tr.flat": ex.tr.flat, "tr.flat_grad": ex.tr.flat_grad}
    groups = list(ex._b.groups) + [g for g, _ in ex.emb_groups]
    for tag, objs in (("linear", ex._b.linears), ("group", groups)):
        for i, L in enumerate(objs):
            for a in ("W", "Wt", "Wm", "A", "At", "B", "Bt", "bias"):
                out[f"{tag}{i}.{a}"] = getattr(L, a)
    for i, L in enumerate(ex._b.linears):
        for a, t in zip(("Wg", "bg", "Bg"), L._geglu or ()):
            out[f"linear{i}.geglu.{a}"] = t
    for k, layers in enumerate(list(ex.blocks) + [ex.mid]):
        for j, l in enumerate(layers):
            cws = {"cw": l.cw} if isinstance(l, _Conv) else {"conv1": l.blk.conv1, "conv2": l.blk.conv2} if isinstance(l, _Res) else {}
            for n, cw in cws.items():
                out.update({f"block{k}.{j}.{n}.{a}": getattr(cw, a) for a in ("Wp", "Wd", "bias")})
                out.update({f"block{k}.{j}.{n}.phase.{kind}": t for kind, t in cw._phase.items()})
    for i, n in enumerate(ex._b.norms):
        out[f"norm{i}.gamma"], out[f"norm{i}.beta"] = n.gamma, n.beta
    return {k: t for k, t in out.items() if t is not None}


def test_no_packed_tensor_of_the_control_executor_moves_across_load_state_dict():
    _need_gpu()
    from oracle import arch
    from ctrlora_amd import hip
    from ctrlora_amd.engine.nets import _Conv
    from ctrlora_amd.engine.packing import Conv3W
    from tests.test_gpu_flags import _fixture_inputs, _model
    _, meta, cfg, inp, sd_cn, sd_un = _fixture_inputs()
    m = _model(True, True, BF, sd_cn, sd_un, lr=meta["lr"])
    opt = m.configure_optimizers()
    cu = lambda v: v.cuda()
    opt.zero_grad()
    loss, _ = m.p_losses(cu(inp["z"]), {"c_crossattn": [cu(inp["ctx"])], "c_concat": [cu(inp["hint_z"])]}, cu(inp["t"]),
                         noise=cu(inp["noise"]))
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    ex = m.control_model.executor()
    before = {k: t.data_ptr() for k, t in _packed_tensors(ex).items()}
    t2 = [k for k in before if k.endswith(".phase.t2")]
    assert len(t2) == 3                                           # the three Downsample convs
    other = arch.make_state(arch.controlnet_shapes(cfg), meta["seed"] + 1)
    m.control_model.load_state_dict(other, strict=True)
    torch.cuda.synchronize()
    assert m.control_model.executor() is ex
    after = {k: t.data_ptr() for k, t in _packed_tensors(ex).items()}
    moved = sorted(k for k in set(before) | set(after) if before.get(k) != after.get(k))
    assert not moved, moved
    for k, layers in enumerate(ex.blocks):
        for l in layers:
            if isinstance(l, _Conv) and l.mode == hip.CONV_S2:
                n = f"input_blocks.{k}.0.op"
                fresh = Conv3W(other[n + ".weight"], other[n + ".bias"], BF, "cuda", True)
                assert torch.equal(l.cw._phase["t2"], fresh.phase_weights("t2")), n
