"""ControlNetFinetune's norm_trainable / zero_trainable switches, the part that needs no GPU: the mirror's name filter and
the engine's flat trainable layout against the list recorded from the UNMODIFIED reference (tests/golden/flags_tiny.pt,
written by tests/golden/make_golden_flags.py), the oracle's gradients against the recorded ones, and the data-parallel
exchange on a layout with empty backward stages."""
import hashlib
import multiprocessing as mp
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist

from tests.flags_common import COMBOS, combo_key, digest_close, load_flags_golden, netcfg, sample_idx, selected
from tests.util import ROOT, rel_l2
from oracle import arch, ref_model as R


def _mirror(nt, zt, **extra):
    import yaml
    from ldm.util import instantiate_from_config
    with open(os.path.join(ROOT, "configs", "ctrlora_finetune_sd15_rank32.yaml")) as f:
        cfg = yaml.safe_load(f)["model"]
    p = cfg["params"]
    for k in ("control_stage_config", "unet_config"):
        p[k]["params"].update(model_channels=64, context_dim=96)
    p["control_stage_config"]["params"].update(lora_rank=32, norm_trainable=nt, zero_trainable=zt, **extra)
    p["first_stage_config"] = {"target": "torch.nn.Identity"}
    p["cond_stage_config"] = {"target": "torch.nn.Identity"}
    return instantiate_from_config(cfg)


@pytest.mark.parametrize("nt,zt", COMBOS)
def test_mirror_name_filter_equals_the_reference_list(nt, zt):
    gold = load_flags_golden()["combos"][combo_key(nt, zt)]
    names = _mirror(nt, zt).trainable_names()
    assert names == gold["trainable_names"]          # same tensors, the reference's order
    assert all(selected(n, nt, zt) for n in names)
    assert len(names) == 164 + 26 * zt + 56 * nt     # 164 LoRA + 26 zero-conv + 56 norm tensors


def test_flags_are_ignored_without_lora_as_in_the_reference():
    m = _mirror(False, False, ft_with_lora=False)
    names = m.trainable_names()
    assert sorted(names) == sorted(n for n, _ in m.control_model.named_parameters())
    assert any("zero_convs" in n for n in names) and any("norm" in n for n in names)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("nt,zt", COMBOS)
def test_layout_only_executor_holds_exactly_the_filtered_set(nt, zt, dtype):
    from ctrlora_amd.engine import ControlNetE
    from ctrlora_amd.engine.packing import rup
    cfg = arch.TINY
    gold = load_flags_golden()["combos"][combo_key(nt, zt)]
    shapes = arch.controlnet_shapes(cfg)
    ex = ControlNetE(arch.make_state(shapes, 1), netcfg(cfg), dtype, torch.device("cpu"), layout_only=True,
                     norm_trainable=nt, zero_trainable=zt)
    names = [t.name for t in ex.tr.items]
    assert sorted(names) == sorted(gold["trainable_names"]) and len(set(names)) == len(names)
    assert not any(("zero_convs" in n or "middle_block_out" in n) and not zt for n in names)
    assert not any("norm" in n and "lora_layer" not in n and not nt for n in names)
    numel = lambda n: int(torch.tensor(shapes[n]).prod())
    assert sum(t.master.numel() for t in ex.tr.items) == sum(numel(n) for n in gold["trainable_names"])
    assert ex.tr.numel == sum(rup(numel(n), 64) for n in names) == ex.tr.flat_grad.numel()   # nothing but 64-float padding
    # the spans the backward reports still tile the (smaller) buffer in order; stages without a trainable are dropped
    order = ex.backward_stage_order()
    assert order[0][0] == 0 and order[-1][1] == ex.tr.numel
    assert all(a[1] == b[0] and a[1] > a[0] for a, b in zip(order, order[1:] + [(ex.tr.numel, 0)]))
    empty = [k for k, s in enumerate(ex.stage_spans) if s[1] == s[0]]
    if not zt:
        assert 0 in empty                            # stage 0 = the frozen input conv + a frozen zero conv
        assert len(order) == len(ex.stage_spans) + 1 - len(empty)
    else:
        assert not empty
    # every tensor lies in the span of the stage that finalises it
    covered = sorted((s, e) for s, e in order)
    for t in ex.tr.items:
        assert any(s <= t.offset and t.offset + t.master.numel() <= e for s, e in covered), t.name
    assert all(t.offset >= order[-1][0] for t in ex.tr.items if t.name.startswith("time_embed."))
    # frozen norms / zero convs kept their loaders (reload_frozen) and carry no trainable handle
    assert all((w.tg is None) for w in ex._b.norms) == (not nt)
    assert all((z.tW is None and z.tb is None) == (not zt) for z in ex.zero)


# sha256 of repr((names + offsets, stage_spans, time_span, backward_stage_order(), numel)) of the layout-only executor built by
# the commit BEFORE the flags reached the engine (df63312), with every key of oracle.arch.controlnet_shapes present
PARENT_LAYOUT = {
    ("tiny", torch.float32): "1fb241ece06d4a312e154ab9d2d39692ab9fcf19cc279fad1e86a0f676716b49",
    ("tiny", torch.bfloat16): "806f651c9d5fb8a4c88494d3dc2d51b717076eaba8c68e92001308e1e824cbf1",
    ("sd15", torch.float32): "9c632a17272b70763fc5b784637cd4c1e538e92bbc9f4a282e4b6d9b0cbba919",
    ("sd15", torch.bfloat16): "4655e43449e2e688137d996cc63fe3f5cf0983381105d90e300d77f4518c9c0c",
}


@pytest.mark.parametrize("name,dtype", list(PARENT_LAYOUT))
def test_default_flags_keep_the_parent_layout(name, dtype):
    from ctrlora_amd.engine import ControlNetE
    cfg = arch.TINY if name == "tiny" else arch.SD15
    sd = {k: torch.zeros(s) for k, s in arch.controlnet_shapes(cfg).items()}
    for kw in ({}, dict(norm_trainable=True, zero_trainable=True)):
        ex = ControlNetE(sd, netcfg(cfg), dtype, torch.device("cpu"), layout_only=True, **kw)
        desc = repr(([(t.name, t.offset) for t in ex.tr.items], ex.stage_spans, ex.time_span, ex.backward_stage_order(),
                     ex.tr.numel))
        assert len(ex.tr.items) == 246
        assert hashlib.sha256(desc.encode()).hexdigest() == PARENT_LAYOUT[(name, dtype)]


@pytest.mark.parametrize("nt,zt", COMBOS)
def test_oracle_gradients_restricted_to_the_list_match_the_reference(nt, zt):
    g = load_flags_golden()
    meta, gold = g["meta"], g["combos"][combo_key(nt, zt)]
    cfg = arch.TINY
    from tests.golden.make_golden import inputs_for
    inp = inputs_for(cfg, meta["B"], meta["H"], meta["seed"])
    sd_cn = arch.make_state(arch.controlnet_shapes(cfg), meta["seed"])
    sd_un = arch.make_state(arch.unet_shapes(cfg), meta["seed"])
    tr = [k for k in sd_cn if selected(k, nt, zt)]
    assert sorted(tr) == sorted(gold["trainable_names"])
    init = {k: v.clone() for k, v in sd_cn.items()}
    for k in tr:
        sd_cn[k].requires_grad_(True)
    loss, eps = R.p_losses(sd_cn, sd_un, cfg, R.make_schedule(), inp["z"], inp["t"], inp["ctx"], inp["hint_z"], inp["noise"])
    assert rel_l2(eps, gold["eps"]) < 2e-5
    assert abs(float(loss.detach()) - gold["loss"]) < 1e-5 * abs(gold["loss"])
    loss.backward()
    for k in tr:
        gr = sd_cn[k].grad
        digest_close(gr, gold["grad_digest"][k], 2e-4)
        s = gold["grad_vals"][k]
        assert s["l2"] > 0.0
        assert rel_l2(gr.flatten()[sample_idx(gr.numel(), meta["n_sampled"])], s["vals"]) < 2e-4, k
    for k, d in gold["adamw_digest"].items():
        p = sd_cn[k].detach()
        newp, _, _ = R.adamw_step(p, sd_cn[k].grad, torch.zeros_like(p), torch.zeros_like(p), 1, meta["lr"])
        digest_close(newp, d, 1e-5)
    # what the reference left alone: recorded after its optimizer step, equal to the key-addressed draw
    assert any("norm" in k for k in gold["frozen_digest"]) == (not nt)
    assert any("zero_convs" in k for k in gold["frozen_digest"]) == (not zt)
    for k, d in gold["frozen_digest"].items():
        assert k not in tr and d["after"] == d["initial"]
        digest_close(init[k], d["after"], 0.0)


def test_optimizer_state_of_other_flags_is_refused():
    """FusedAdamW.load_state_dict: a state saved with more (or fewer) trainables than the model has must not load."""
    from ctrlora_amd.engine import ControlNetE
    from ctrlora_amd.train import FusedAdamW
    cfg = arch.TINY
    sd = arch.make_state(arch.controlnet_shapes(cfg), 1)
    mk = lambda nt: ControlNetE(sd, netcfg(cfg), torch.float32, torch.device("cpu"), layout_only=True, norm_trainable=nt)
    full, lean = mk(True), mk(False)
    # (the constructor launches nothing: a layout_only executor on the CPU is enough)
    opts = {key: FusedAdamW([torch.nn.Parameter(ex.tr.flat)], [ex]) for key, ex in (("full", full), ("lean", lean))}
    st_full, st_lean = opts["full"].state_dict(), opts["lean"].state_dict()
    st_full["step"] = st_lean["step"] = 7
    opts["full"]._m[0].fill_(3.0)
    with pytest.raises(KeyError, match="optimizer state lacks"):
        opts["full"].load_state_dict(st_lean)
    with pytest.raises(KeyError, match="does not train"):
        opts["lean"].load_state_dict(st_full)
    # a refused state changed nothing: neither the step counter nor a moment
    assert opts["full"]._step == 0 and opts["lean"]._step == 0
    assert bool((opts["full"]._m[0] == 3.0).all())
    opts["lean"].load_state_dict(st_lean)
    assert opts["lean"]._step == 7


# ------------------------------------------------------------------ DP-2 == one large batch, LoRA-only layout

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _dp_equiv_worker(rank, world, port, q):
    """tests/test_parallel_gloo.py:_dp_equiv_worker with both flags off: the flat buffer holds the LoRA factors only and
    several backward stages (the input conv's, the Downsamples', the ResBlock-only ones of the bf16 layout) have no span."""
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    try:
        from ctrlora_amd.engine import ControlNetE
        from ctrlora_amd.parallel import GradAllReduce
        from ctrlora_amd.trainer import Trainer
        from tests.golden.make_golden import inputs_for
        cfg = arch.TINY
        sd_cn = arch.make_state(arch.controlnet_shapes(cfg), 40 + rank)
        sd_un = arch.make_state(arch.unet_shapes(cfg), 40)
        holder = torch.nn.ParameterDict({k.replace(".", "_"): torch.nn.Parameter(v.clone()) for k, v in sd_cn.items()})
        Trainer.broadcast_module_state(holder)
        sd_cn = {k: holder[k.replace(".", "_")].detach().clone() for k in sd_cn}
        ref0 = arch.make_state(arch.controlnet_shapes(cfg), 40)
        same_start = all(torch.equal(sd_cn[k], ref0[k]) for k in sd_cn)
        # the bf16 engine's layout (grouped emb_layers factors at the tail): the one with the most empty stages
        ex = ControlNetE(sd_cn, netcfg(cfg), torch.bfloat16, torch.device("cpu"), layout_only=True,
                         norm_trainable=False, zero_trainable=False)
        dp = GradAllReduce([ex], bucket_bytes=64 << 10)
        B = 2 * world
        inp = inputs_for(cfg, B, 8, 77)
        sl = slice(rank * 2, rank * 2 + 2)
        sched = R.make_schedule()

        def grads_of(rows):
            sd = {k: v.clone().requires_grad_(selected(k, False, False)) for k, v in sd_cn.items()}
            loss, _ = R.p_losses(sd, sd_un, cfg, sched, inp["z"][rows], inp["t"][rows], inp["ctx"][rows],
                                 inp["hint_z"][rows], inp["noise"][rows])
            loss.backward()
            return float(loss), {k: v.grad for k, v in sd.items() if v.grad is not None}

        _, g_local = grads_of(sl)
        assert sorted(g_local) == sorted(t.name for t in ex.tr.items)
        for t in ex.tr.items:
            t.grad.copy_(g_local[t.name])
        reported = []
        hook = ex.on_stage_done
        ex.on_stage_done = lambda s, e: (reported.append((s, e)), hook(s, e))
        # what ControlNetE.bwd does: one _done per stage, in backward order, silent for a stage without a span.  (Restated here,
        # as tests/test_parallel_gloo.py restates it: a layout-only executor cannot run a backward, so `reported ==
        # backward_stage_order()` below checks the two descriptions of the plan against each other, not the hook itself.  The
        # real ControlNetE._done firing on the reduced layout is covered on the GPU: tests/test_gpu_flags.py, the segmented
        # graph step and the SD1.5-width bucket row.)
        nb = len(ex.blocks)
        for span in [ex.stage_spans[nb]] + [ex.stage_spans[k] for k in range(nb - 1, -1, -1)] + [ex.time_span]:
            if span[1] > span[0]:
                ex.on_stage_done(span[0], span[1])
        dp.on_backward_done()
        dp.wait()
        n_empty = sum(1 for s in ex.stage_spans if s[1] == s[0])
        tiled = reported == ex.backward_stage_order() and reported[0][0] == 0 and reported[-1][1] == ex.tr.numel and \
            all(a[1] == b[0] for a, b in zip(reported, reported[1:]))
        _, g_full = grads_of(slice(0, B))
        worst = max(float((t.grad / world - g_full[t.name]).norm() / (g_full[t.name].norm() + 1e-30)) for t in ex.tr.items)
        p_new, _, _ = R.adamw_step(ex.tr.flat, ex.tr.flat_grad / world, torch.zeros_like(ex.tr.flat),
                                   torch.zeros_like(ex.tr.flat), 1, 1e-3)
        gathered = [torch.empty_like(p_new) for _ in range(world)]
        dist.all_gather(gathered, p_new)
        in_sync = all(torch.equal(gathered[0], g) for g in gathered)
        q.put((rank, same_start, worst, dp.launches, in_sync, len(ex.tr.items), n_empty, tiled,
               dp.launched_bytes == 4 * ex.tr.numel))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_dp2_equals_single_large_batch_on_the_lora_only_layout_gloo():
    """Both flags off, two gloo ranks, the real GradAllReduce on the engine's reduced layout: stages without a trainable
    report nothing (on every rank alike), the remaining spans tile the buffer, every byte is exchanged once, and after the
    exchange every rank holds world * (full-batch gradient)."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_equiv_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=540) for _ in range(2)]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for rank, same_start, worst, launches, in_sync, n, n_empty, tiled, all_bytes in res:
        assert same_start
        assert n == 164
        assert n_empty >= 4, n_empty         # input conv, 3 Downsamples (+ the ResBlock-only stages of the deepest level)
        assert tiled
        assert worst < 2e-5, (rank, worst)   # the bound of test_dp2_equals_single_large_batch_on_the_engine_layout_gloo
        assert launches >= 2 and all_bytes
        assert in_sync
