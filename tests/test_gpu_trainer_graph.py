"""`Trainer(graph_step=...)` on an MI355X: the optimizer step replayed from hipGraphs follows the eager loop's trajectory.

Model: bench.build_model(..., tiny=True) (width 64, context 96, rank 32), B = 2, latent 16 x 16 (the smallest grid with all four
levels), learning rate 1e-3; batches are distinct dicts with ready z, ctx, hint_z and the model instance's get_input hands them
through.  Every leg builds a twin model from the same seed and calls torch.manual_seed right before fit; log_every_n_steps=1, so
trainer.logged holds every optimizer step's loss.

Gate ("same trajectory"), the one of tests/test_gpu_parity.py::test_graphed_train_step_matches_eager_steps: every logged loss within
1e-4 relative and rel-L2 < 1e-4 on EVERY control_model parameter, in fp32.  In bf16 the comparator is measured in the test: the
eager leg runs twice from one seed, that spread is the floor (the weight gradients are accumulated with atomics), and graph against
eager may be 2 x the spread or the fp32 gate, whichever is larger.

Every test also proves that the graph ran: graph_replays == optimizer steps - graph_eager_steps, graph_eager_steps <= 3,
int(optimizer._step) == trainer.global_step.
"""
import importlib.util
import os
import sys
import time

import pytest
import torch

from tests.util import ROOT, rel_l2

pytestmark = pytest.mark.gpu

B, H, CTX_DIM, SEED, GATE = 2, 16, 96, 7, 1e-4


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _batches(n, seed=5):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g).cuda()
    return [dict(z=mk(B, 4, H, H), ctx=mk(B, 77, CTX_DIM), hint_z=mk(B, 4, H, H) * 0.9) for _ in range(n)]


def _model(loss_type=None):
    import bench
    m = bench.build_model("ctrlora_finetune_sd15_rank128.yaml", 0, tiny=True)
    m.learning_rate = 1e-3
    m.get_input = lambda batch, k, *a, **kw: (batch["z"], {"c_crossattn": [batch["ctx"]], "c_concat": [batch["hint_z"]]})
    if loss_type is not None:
        m.loss_type = loss_type
    return m


def _fit(batches, graph_step, steps, acc=1, precision=32, callbacks=(), ckpt_path=None, rng_state=None, model=None):
    from ctrlora_amd.trainer import Trainer
    m = _model() if model is None else model
    tr = Trainer(max_steps=steps, accumulate_grad_batches=acc, precision=precision, callbacks=list(callbacks),
                 default_root_dir="run", log_every_n_steps=1, graph_step=graph_step)
    torch.manual_seed(SEED)
    if rng_state is not None:
        torch.cuda.set_rng_state(rng_state)       # a resumed leg continues the uninterrupted leg's stream of t and noise
    tr.fit(m, batches, ckpt_path=ckpt_path)
    torch.cuda.synchronize()
    return tr


def _params(tr):
    return {k: v.detach().float().cpu().clone() for k, v in tr.model.control_model.named_parameters()}


def _losses(tr):
    return [v for _, v in tr.logged]


def _spread(a_losses, a_params, b_losses, b_params):
    """(largest relative loss difference over the steps, largest rel-L2 over all control_model parameters)."""
    assert len(a_losses) == len(b_losses) and set(a_params) == set(b_params)
    dl = max(abs(x - y) / abs(y) for x, y in zip(a_losses, b_losses))
    dp = max(rel_l2(a_params[k], b_params[k]) for k in b_params)
    return dl, dp


def _assert_same(what, got, want, gate_l=GATE, gate_p=GATE):
    dl, dp = _spread(got[0], got[1], want[0], want[1])
    print(f"[trainer graph] {what}: max rel loss diff {dl:.3e} (gate {gate_l:.3e}), max param rel-L2 {dp:.3e} (gate {gate_p:.3e})")
    assert dl < gate_l and dp < gate_p, (what, dl, dp)


def _assert_graph_ran(tr, steps, mode="one"):
    assert tr.global_step == steps and int(tr.optimizer._step) == tr.global_step
    assert tr.graph_mode == mode
    assert tr.graph_eager_steps <= 3 and tr.graph_replays == steps - tr.graph_eager_steps and tr.graph_replays > 0
    assert not torch.cuda.is_current_stream_capturing()


_REF = {}


def _eager_ref(precision, acc):
    """The eager loop's trajectory (losses, parameters, device RNG state after it), computed once per form."""
    key = (precision, acc)
    if key not in _REF:
        n = 6 if acc == 1 else 4
        tr = _fit(_batches(n * acc), False, n, acc=acc, precision=precision)
        assert tr.graph_mode == "off" and tr.graph_replays == 0 and int(tr.optimizer._step) == n
        losses = _losses(tr)
        assert len(losses) == n and len(set(losses)) == n, f"the losses must differ from step to step: {losses}"
        _REF[key] = (losses, _params(tr))
    return _REF[key]


@pytest.fixture(autouse=True)
def _workdir(tmp_path, monkeypatch):
    _need_gpu()
    monkeypatch.chdir(tmp_path)          # configure_optimizers writes ./tmp/finetune_trainable_params.txt, the trainer ./run


@pytest.mark.parametrize("precision", [32, 16], ids=["fp32", "bf16"])
def test_same_trajectory_as_eager(precision):
    """Six optimizer steps over six distinct batches, graph_step=True against False."""
    want = _eager_ref(precision, 1)
    gate_l = gate_p = GATE
    if precision == 16:
        again = _fit(_batches(6), False, 6, precision=16)
        fl, fp = _spread(_losses(again), _params(again), *want)
        print(f"[trainer graph] bf16 eager against eager, same seed: max rel loss diff {fl:.3e}, max param rel-L2 {fp:.3e}")
        gate_l, gate_p = max(2 * fl, GATE), max(2 * fp, GATE)
    tr = _fit(_batches(6), True, 6, precision=precision)
    _assert_graph_ran(tr, 6)
    assert tr.graph_eager_steps == 2, "two warm steps, each on its own batch"
    losses = _losses(tr)
    assert len(set(losses)) == 6, f"identical losses would hide a batch that is consumed twice: {losses}"
    _assert_same(f"graph against eager, precision {precision}", (losses, _params(tr)), want, gate_l, gate_p)


def test_accumulation():
    """accumulate_grad_batches=2 over eight micro-batches: four optimizer steps in both legs."""
    want = _eager_ref(32, 2)
    tr = _fit(_batches(8), True, 4, acc=2)
    _assert_graph_ran(tr, 4)
    step = tr._graph_step_obj
    assert step.accumulate and step.grad_scale == 0.5 and step.g_z is not None and step.g_b is not None
    _assert_same("graph against eager, acc 2", (_losses(tr), _params(tr)), want)


def test_segmented_form_on_one_rank():
    """The data-parallel structure on one rank with a counting identity in place of the all-reduce: same trajectory, the slices
    handed to reduce_fn over one optimizer step tile the flat gradient buffer exactly once, and only final micro-steps call it."""
    want = _eager_ref(32, 2)
    state = {"micro": 0, "model": None}
    calls = []

    def counting_identity(buf):
        flat = state["model"].control_model.executor().tr.flat_grad
        assert buf.dtype == torch.float32 and buf.is_contiguous()
        calls.append((state["micro"], (buf.data_ptr() - flat.data_ptr()) // 4, buf.numel(), flat.numel()))
        return None

    class Count:
        def on_train_batch_end(self, trainer, module, outputs, batch, batch_idx):
            state["micro"] += 1

    state["model"] = m = _model()
    tr = _fit(_batches(8), dict(split_graphs="segmented", bucket_bytes=256 << 10, reduce_fn=counting_identity), 4, acc=2,
              callbacks=[Count()], model=m)
    _assert_graph_ran(tr, 4, mode="segmented")
    assert m.dp is None or not m.dp.enabled
    assert calls and all(c[0] % 2 == 1 for c in calls), "reduce_fn was called on a non-final micro-step"
    for s in range(4):
        spans = sorted((lo, n) for mi, lo, n, _ in calls if mi == 2 * s + 1)
        total = calls[0][3]
        pos = 0
        for lo, n in spans:
            assert lo == pos and n > 0, f"optimizer step {s + 1}: slices {spans} do not tile [0, {total})"
            pos += n
        assert pos == total, f"optimizer step {s + 1}: slices {spans} do not tile [0, {total})"
    per_step = [sum(1 for c in calls if c[0] == 2 * s + 1) for s in range(4)]
    print(f"[trainer graph] segmented: slices per optimizer step {per_step}, {len(tr._graph_step_obj.segments)} segment graphs")
    assert per_step[-1] > 1 and len(tr._graph_step_obj.segments) > 1, "one bucket only: the segmented form was not exercised"
    _assert_same("segmented graph against eager, acc 2", (_losses(tr), _params(tr)), want)


_FORM_REF = {}


def _form_model():
    m = _model().cuda().train()
    m.set_engine_dtype(torch.float32)
    return m, m.configure_optimizers()


def _form_batches(acc):
    """Three optimizer steps' worth of distinct micro-batches as (z, ctx, hint, t, noise) tuples."""
    g = torch.Generator().manual_seed(11)
    out = []
    for b in _batches(3 * acc, seed=9):
        t = torch.randint(0, 1000, (B,), generator=g).cuda()
        out.append((b["z"], b["ctx"], b["hint_z"], t, torch.randn(B, 4, H, H, generator=g).cuda()))
    return out


def _form_eager_ref(acc):
    """Three optimizer steps launched eagerly through autograd (acc micro-batches each, every loss scaled by 1 / acc for the
    backward as the trainer does): (every micro-step's loss, every control_model parameter).  Computed once per acc."""
    if acc not in _FORM_REF:
        m, opt = _form_model()
        losses = []
        for i, (z, ctx, hint, t, noise) in enumerate(_form_batches(acc)):
            if i % acc == 0:
                opt.zero_grad()
            loss, _ = m.p_losses(z, {"c_crossattn": [ctx], "c_concat": [hint]}, t, noise=noise)
            (loss / acc).backward()
            losses.append(float(loss.detach()))
            if i % acc == acc - 1:
                opt.step()
        torch.cuda.synchronize()
        assert int(opt._step) == 3 and len(set(losses)) == 3 * acc
        _FORM_REF[acc] = (losses, {k: v.detach().float().cpu().clone() for k, v in m.control_model.named_parameters()})
    return _FORM_REF[acc]


@pytest.mark.parametrize("accumulate", [False, True], ids=["acc1", "acc2"])
@pytest.mark.parametrize("split", [False, "two", "segmented"], ids=["one", "two", "segmented"])
def test_every_capture_form_follows_eager_and_holds_the_planned_pieces(split, accumulate):
    """GraphedTrainStep in each of its six (mode, accumulate) forms, used the way the trainer uses it: optimizer step 1 is
    launched by eager() to warm the allocations, capture() records, steps 2 and 3 are replays.  The trajectory is the eager
    one (the fp32 gates of test_same_trajectory_as_eager), the graphs that exist are the ones capture_plan lists, and in the
    exchanging modes the slices handed to reduce_fn tile every flat gradient buffer exactly once per optimizer step."""
    from ctrlora_amd.train import GraphedTrainStep, capture_plan
    acc = 2 if accumulate else 1
    mode = split or "one"
    want = _form_eager_ref(acc)
    m, opt = _form_model()
    handed = []

    def recording_identity(buf):
        assert buf.dtype == torch.float32 and buf.is_contiguous()
        for i, ex in enumerate(opt.executors):
            lo = (buf.data_ptr() - ex.tr.flat_grad.data_ptr()) // 4
            if 0 <= lo < ex.tr.flat_grad.numel():
                handed.append((i, lo, lo + buf.numel()))
                return None
        raise AssertionError("reduce_fn was handed memory outside every flat gradient buffer")

    batches = _form_batches(acc)
    gs = GraphedTrainStep(m, opt, *batches[0], warmup=0, capture=False, split_graphs=split, bucket_bytes=256 << 10,
                          reduce_fn=recording_identity, accumulate=accumulate, grad_scale=1.0 / acc)
    assert gs.mode == mode and not gs.captured and gs.segments == []
    losses, per_step = [], []
    for step in range(3):
        if step == 1:
            gs.capture()
            assert gs.captured and not torch.cuda.is_current_stream_capturing()
            assert handed == [], "capturing handed a slice to reduce_fn"
        for k in range(acc):
            args, first, last = batches[step * acc + k], k == 0, k == acc - 1
            if step == 0:
                losses.append(float(gs.eager(*args, first=first, last=last)[2]))
            elif accumulate:
                losses.append(float(gs.micro(*args, first=first, last=last)[2]))
            else:
                losses.append(float(gs(*args)))
            assert last or handed == [], "reduce_fn was called on a non-final micro-step"
        per_step.append(sorted(handed))
        handed.clear()
    torch.cuda.synchronize()
    assert int(opt._step) == 3

    # the pieces: what capture_plan lists is what exists
    plan = capture_plan(mode, accumulate)
    kinds = [p.kind for p in plan]
    (f,) = [p for p in plan if p.kind == "F"]
    assert (gs.g_z is not None) == accumulate == ("Z" in kinds)
    assert (gs.g_b is None) == (mode == "one" and not accumulate) == ("B" not in kinds) == f.with_opt
    tags = [tag for _, tag, _, _ in gs.segments]
    if mode == "segmented":
        assert f.segmented and len(gs.segments) >= 3
        assert all(isinstance(t, int) for t in tags[:-1]) and tags[-1] == "tails"
    else:
        assert not f.segmented and len(gs.segments) == 1 and tags == [f.tag]
    # the exchange: nothing on one rank in one graph, else every slice of every buffer once per optimizer step
    for step, spans in enumerate(per_step):
        if mode == "one":
            assert spans == []
            continue
        for i, ex in enumerate(opt.executors):
            pos = 0
            for _, lo, hi in [s for s in spans if s[0] == i]:
                assert lo == pos and hi > lo, f"optimizer step {step + 1}: slices {spans} do not tile executor {i}'s buffer"
                pos = hi
            assert pos == ex.tr.flat_grad.numel(), f"optimizer step {step + 1}: slices {spans} do not tile executor {i}'s buffer"
    if mode == "segmented":
        assert len(per_step[1]) == len(per_step[2]) > 1, "one bucket only: the segmented exchange was not exercised"
    print(f"[trainer graph] form ({mode}, acc {acc}): {len(gs.segments)} F graph(s), slices per step {[len(s) for s in per_step]}")
    got = (losses, {k: v.detach().float().cpu().clone() for k, v in m.control_model.named_parameters()})
    _assert_same(f"form ({mode}, acc {acc}) against eager", got, want)


def test_work_between_replays():
    """After optimizer step 3 a callback samples with DDIM in eval mode (both legs); training goes on to step 6 on the eager
    trajectory and both legs' samples agree: the sampler saw the replayed weights and did not disturb the capture."""
    from cldm.ddim_hacked import DDIMSampler
    batches = _batches(6)

    class SampleAt3:
        def __init__(self):
            self.sample = None

        def on_train_batch_end(self, trainer, module, outputs, batch, batch_idx):
            if trainer.global_step != 3 or self.sample is not None:
                return
            cond = {"c_concat": [batches[0]["hint_z"]], "c_crossattn": [batches[0]["ctx"]]}
            module.eval()
            with torch.no_grad():
                x, _ = DDIMSampler(module).sample(4, B, (4, H, H), cond, verbose=False)
            self.sample = x.detach().float().cpu().clone()
            module.train()

    legs = {}
    for name, gs in (("eager", False), ("graph", True)):
        cb = SampleAt3()
        tr = _fit(batches, gs, 6, callbacks=[cb])
        assert cb.sample is not None and torch.isfinite(cb.sample).all()
        legs[name] = (tr, cb.sample)
    tr = legs["graph"][0]
    _assert_graph_ran(tr, 6)
    assert tr.graph_replays == 4
    _assert_same("graph against eager with sampling after step 3", (_losses(tr), _params(tr)),
                 (_losses(legs["eager"][0]), _params(legs["eager"][0])))
    d = rel_l2(legs["graph"][1], legs["eager"][1])
    print(f"[trainer graph] DDIM samples after step 3, graph against eager: rel-L2 {d:.3e}")
    assert d < GATE
    # the sampler changed nothing the plain run would not have: steps 1-3 of the plain eager reference (the sampler's x_T draw
    # moves the device generator, so later steps legitimately differ from it)
    plain = _eager_ref(32, 1)[0]
    assert all(abs(a - b) <= GATE * abs(b) for a, b in zip(_losses(tr)[:3], plain[:3]))


@pytest.mark.parametrize("resume_graph", [True, False], ids=["graph-graph", "graph-eager"])
def test_resume_across_modes(resume_graph, tmp_path):
    """Three replayed steps, a checkpoint, a fresh model resumed for three more (with the graph / eagerly) == six eager steps."""
    want = _eager_ref(32, 1)
    batches = _batches(6)
    a = _fit(batches[:3], True, 3)
    _assert_graph_ran(a, 3)
    rng = torch.cuda.get_rng_state()
    ck = str(tmp_path / "three.ckpt")
    a.save_checkpoint(ck)
    saved = torch.load(ck, map_location="cpu", weights_only=False)
    assert sorted(saved) == ["epoch", "global_step", "optimizer_states", "state_dict"] and saved["global_step"] == 3
    assert saved["optimizer_states"][0]["step"] == 3 and saved["optimizer_states"][0]["format"] == "by_name"
    del a
    b = _fit(batches[3:], resume_graph, 6, ckpt_path=ck, rng_state=rng)
    assert b.global_step == 6 and int(b.optimizer._step) == 6
    if resume_graph:
        # the resumed fit warms and captures again: two eager steps, one replay
        assert b.graph_mode == "one" and b.graph_eager_steps == 2 and b.graph_replays == 1
    else:
        assert b.graph_mode == "off" and b.graph_replays == 0
    losses = want[0][:3] + _losses(b)
    assert [s for s, _ in b.logged] == [4, 5, 6]
    _assert_same(f"3 graph steps + 3 resumed ({'graph' if resume_graph else 'eager'}) against 6 eager", (losses, _params(b)), want)


def test_refusals():
    """loss_type 'l1' is refused before any step with the reason; nothing is left capturing and an eager fit still works."""
    from ctrlora_amd.trainer import Trainer
    m = _model(loss_type="l1")
    before = {k: v.detach().clone() for k, v in m.control_model.named_parameters()}
    tr = Trainer(max_steps=2, default_root_dir="run", log_every_n_steps=1, graph_step=True)
    with pytest.raises(ValueError, match="graph_step refused.*loss_type is 'l1'"):
        tr.fit(m, _batches(2))
    assert tr.global_step == 0 and tr.optimizer is None and tr.graph_replays == 0 and tr.graph_eager_steps == 0
    assert not torch.cuda.is_current_stream_capturing()
    assert all(torch.equal(v.detach().cpu(), before[k].cpu()) for k, v in m.control_model.named_parameters())
    # the pre-training LDM keeps its eager loop
    from ctrlora_amd.trainer import graph_step_refusal
    import bench
    pre = bench.build_model("ctrlora_pretrain_sd15_9tasks_rank128.yaml", 0, tiny=True)
    assert "pre-training" in graph_step_refusal(pre)
    del pre
    ok = _fit(_batches(2), False, 2, model=m)
    assert ok.global_step == 2 and int(ok.optimizer._step) == 2 and all(v == v and v > 0 for v in _losses(ok))
    assert not torch.cuda.is_current_stream_capturing()


# ---------------------------------------------------------------------------------------------------- the script, end to end

def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    _need_gpu()
    out = str(tmp_path_factory.mktemp("synth_trainer_graph"))
    mod = _load(os.path.join(ROOT, "tests", "tools", "make_synthetic_assets.py"), "make_synthetic_assets")
    argv, sys.argv = sys.argv, ["make_synthetic_assets.py", "--out", out, "--n", "4"]
    try:
        mod.main()
    finally:
        sys.argv = argv
    mp = pytest.MonkeyPatch()
    try:
        mp.setenv("CTRLORA_SYNTHETIC_TOKENIZER", "1")
        mp.chdir(tmp_path_factory.mktemp("cache_tool_cwd"))
        cache = os.path.join(out, "latents_bf16")
        _load(os.path.join(ROOT, "scripts", "tool_cache_latents.py"), "tool_cache_latents").main(
            ["--dataroot", os.path.join(out, "custom"), "--config", os.path.join(out, "finetune_narrow.yaml"),
             "--sd_ckpt", os.path.join(out, "sd_synth.ckpt"), "--out", cache, "--bs", "4", "--precision", "16"])
    finally:
        mp.undo()
    return out, cache


@pytest.mark.parametrize("cached", [False, True], ids=["live", "latent_cache"])
def test_finetune_script_with_graph(assets, cached, monkeypatch):
    """scripts/train_ctrlora_finetune.py --graph for five steps, from images and from the latent cache."""
    out, cache = assets
    monkeypatch.setenv("CTRLORA_SYNTHETIC_TOKENIZER", "1")
    from ldm.models.autoencoder import AutoencoderKL
    encodes = []
    real_encode = AutoencoderKL.encode
    monkeypatch.setattr(AutoencoderKL, "encode", lambda self, t: (encodes.append(int(t.shape[0])), real_encode(self, t))[1])
    train = _load(os.path.join(ROOT, "scripts", "train_ctrlora_finetune.py"), "train_ctrlora_finetune")
    args = ["--dataroot", os.path.join(out, "custom"), "--config", os.path.join(out, "finetune_narrow.yaml"),
            "--sd_ckpt", os.path.join(out, "sd_synth.ckpt"), "--cn_ckpt", os.path.join(out, "basecn_synth.ckpt"), "--graph", "--bs", "2",
            "--max_steps", "5", "--precision", "16", "--num_workers", "0", "--img_logger_freq", "1000", "--ckpt_logger_freq", "1000",
            "--lr", "1e-4", "-n", "g_cached" if cached else "g_live"] + (["--latent_cache", cache] if cached else [])
    t0 = time.time()
    tr = train.main(args)
    torch.cuda.synchronize()
    print(f"[trainer graph] script --graph ({'latent cache' if cached else 'live first stage'}): {time.time() - t0:.1f} s wall")
    assert tr.global_step == 5 and int(tr.optimizer._step) == 5
    assert tr.graph_mode == "one" and tr.graph_eager_steps <= 3 and tr.graph_replays == 5 - tr.graph_eager_steps and tr.graph_replays > 0
    assert not torch.cuda.is_current_stream_capturing()
    up = [v for k, v in tr.model.state_dict().items() if k.endswith("lora_layer.up.weight")]
    assert up and all(torch.isfinite(v).all() for v in up) and any(float(v.abs().sum()) > 0 for v in up)     # B = 0 at the start
    if cached:
        assert encodes == [], "the first stage encoded during a run from the latent cache"
    else:
        assert encodes == [2, 2] * 5, "live: the target and the condition images of every step, once each"
