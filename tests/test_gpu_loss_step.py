"""The weighted / Huber loss inside engine_train_step on an MI355X, on the tiny models of the flag tests (bench.build_model(tiny=True):
width 64, context 96, rank 32) in fp32 engine mode, B = 2, latent 16 x 16.

Bits are compared, so the fp32 weight gradients run in their opt-in fixed-order form (hip.WGRAD_F32_DETERMINISTIC, as in
tests/test_gpu_latent_cache.py): the default accumulates with float atomics in arrival order and no two steps share their bits.

  (i)   a table of exact ones, and min_snr_gamma at or above the largest SNR (a table of exact ones as well), give the bits of the
        step without weighting: the loss vector and the flat gradient buffer, torch.equal;
  (ii)  the gradient is linear in the table: at t_0 != t_1, g(w[t_0], w[t_1] = a, b) = a g(1, 0) + b g(0, 1), to the rel-L2 the
        project puts on fp32 gradients, 5e-6.  The (1, 0) leg runs twice; if its two gradients are not bit-equal the gate grows by
        three times their rel-L2 (three legs enter the comparison, each carrying that spread) -- it is 0 with the fixed-order form;
  (iii) Huber with a delta beyond every |d| is rho = d^2 / 2: half the l2 step's gradient to the same gate, and 0.5 * loss_l2
        exactly (every term and every partial sum is halved, which is exact in binary floating point);
  (iv)  a pre-training step (ControlPretrainLDM delegates to the same code) with a table runs and satisfies (ii), in the default
        form of the weight gradients.
"""
import pytest
import torch

from tests.util import rel_l2

pytestmark = pytest.mark.gpu

B, H, CTX_DIM, GATE = 2, 16, 96, 5e-6
T0, T1 = 37, 911
FINETUNE, PRETRAIN = "ctrlora_finetune_sd15_rank128.yaml", "ctrlora_pretrain_sd15_9tasks_rank128.yaml"


@pytest.fixture(autouse=True)
def _setup(tmp_path, monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from ctrlora_amd import hip
    hip.lib()
    monkeypatch.setattr(hip, "WGRAD_F32_DETERMINISTIC", True)
    monkeypatch.chdir(tmp_path)          # configure_optimizers writes ./tmp/*_trainable_params.txt


def _inputs():
    g = torch.Generator().manual_seed(23)
    mk = lambda *s: torch.randn(*s, generator=g).cuda()
    return dict(z=mk(B, 4, H, H), ctx=mk(B, 77, CTX_DIM), hint=mk(B, 4, H, H) * 0.9, noise=mk(B, 4, H, H),
                t=torch.tensor([T0, T1]).cuda())


def _finetune(**params):
    import bench
    m = bench.build_model(FINETUNE, 0, tiny=True, mutate=lambda p: p.update(params)).cuda().train()
    m.set_engine_dtype(torch.float32)
    opt = m.configure_optimizers()
    return m, opt, (lambda: m.control_model.executor().tr.flat_grad), {}


def _pretrain(**params):
    import bench

    def mutate(p):
        p.update(params)
        p["control_stage_config"]["params"]["tasks"] = ["hed", "canny"]
    m = bench.build_model(PRETRAIN, 0, tiny=True, mutate=mutate).cuda().train()
    m.set_engine_dtype(torch.float32)
    opt = m.configure_optimizers()
    return m, opt, (lambda: torch.cat([opt.executor.tr.flat_grad, opt.banks["canny"].flat_grad])), dict(task="canny")


def _step(model, inp):
    """One engine_train_step from zeroed gradients: (loss 3-vector, flat gradient), cloned."""
    m, opt, grad, extra = model
    opt.zero_grad()
    out = m.engine_train_step(inp["z"], dict(c_crossattn=[inp["ctx"]], c_concat=[inp["hint"]], **extra), inp["t"], inp["noise"])
    torch.cuda.synchronize()
    g = grad().detach().clone()
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 and bool(torch.isfinite(out).all())
    return out.clone(), g


def _table(m, a, b):
    w = torch.zeros(m.num_timesteps)
    w[T0], w[T1] = a, b
    return w


def _linearity(model, inp, what):
    m = model[0]
    a, b = 0.37, 1.9
    m.set_loss_weights(_table(m, 1.0, 0.0))
    ptr = m.loss_weights.data_ptr()
    o10, g10 = _step(model, inp)
    _, again = _step(model, inp)
    m.set_loss_weights(_table(m, 0.0, 1.0))
    o01, g01 = _step(model, inp)
    m.set_loss_weights(_table(m, a, b))
    oab, gab = _step(model, inp)
    assert m.loss_weights.data_ptr() == ptr
    repeat = 0.0 if torch.equal(g10, again) else rel_l2(again, g10)
    gate = GATE + 3.0 * repeat
    err = rel_l2(gab, a * g10.double() + b * g01.double())
    print(f"[loss step] {what}: linearity rel-L2 {err:.3e} (gate {gate:.3e}; repeat of the (1, 0) leg {repeat:.3e}); "
          f"|g10| {float(g10.norm()):.3e} |g01| {float(g01.norm()):.3e}")
    assert float(g10.norm()) > 0 and float(g01.norm()) > 0 and rel_l2(g10, g01) > 1e-2, "the two legs must be different gradients"
    assert err < gate, (what, err, gate)
    # the unweighted scalars do not move with the table; the weighted one is linear in it too
    assert torch.equal(o10[:2], o01[:2]) and torch.equal(o10[:2], oab[:2])
    want = a * float(o10[2]) + b * float(o01[2])
    assert abs(float(oab[2]) - want) <= 4 * 2.0 ** -24 * abs(want), (float(oab[2]), want)


def test_tables_of_ones_give_the_bits_of_the_unweighted_step():
    inp = _inputs()
    off = _finetune()
    assert off[0].loss_weights is None
    out0, g0 = _step(off, inp)
    _, g0b = _step(off, inp)
    assert torch.equal(g0, g0b), "the comparator itself must be reproducible"
    off[0].set_loss_weights(torch.ones(off[0].num_timesteps))
    out1, g1 = _step(off, inp)
    assert torch.equal(out1, out0) and torch.equal(g1, g0), "a table of exact ones"
    import numpy as np
    acp = np.cumprod(1.0 - off[0].betas.double().cpu().numpy())
    big = _finetune(min_snr_gamma=float(2.0 * (acp / (1.0 - acp)).max()))
    assert torch.equal(big[0].loss_weights, torch.ones_like(big[0].loss_weights))
    out2, g2 = _step(big, inp)
    assert torch.equal(out2, out0) and torch.equal(g2, g0), "min_snr_gamma above the largest SNR"
    # and a table that is not all ones moves both
    five = _finetune(min_snr_gamma=5.0)
    out3, g3 = _step(five, inp)
    assert float(five[0].loss_weights[T0]) < 1.0 and float(five[0].loss_weights[T1]) == 1.0
    assert torch.equal(out3[:2], out0[:2]) and float(out3[2]) < float(out0[2]) and not torch.equal(g3, g0)


def test_gradient_is_linear_in_the_table():
    _linearity(_finetune(), _inputs(), "fine-tune, l2")


def test_gradient_is_linear_in_the_table_with_huber():
    _linearity(_finetune(loss_type="huber", huber_delta=0.5), _inputs(), "fine-tune, Huber delta 0.5")


def test_huber_with_a_large_delta_is_half_the_l2_step():
    inp = _inputs()
    out2, g2 = _step(_finetune(), inp)
    outh, gh = _step(_finetune(loss_type="huber", huber_delta=1e4), inp)
    err = rel_l2(gh, 0.5 * g2.double())
    print(f"[loss step] Huber, delta 1e4 against 0.5 x l2: gradient rel-L2 {err:.3e} (gate {GATE:.1e}); loss {float(outh[2])!r} vs "
          f"0.5 x {float(out2[2])!r}")
    assert err < GATE
    assert torch.equal(outh, 0.5 * out2)
    # a delta inside the residuals is another gradient
    _, gs = _step(_finetune(loss_type="huber", huber_delta=0.5), inp)
    assert rel_l2(gs, 0.5 * g2.double()) > 1e-2


def test_pretraining_step_takes_the_table(monkeypatch):
    """Pre-training forms every weight gradient, the 4-channel input convolution's among them, which the fixed-order form refuses
    (its rows are written eight columns at a time): this test runs the default form and relies on the measured repeat."""
    from ctrlora_amd import hip
    monkeypatch.setattr(hip, "WGRAD_F32_DETERMINISTIC", False)
    model = _pretrain()
    assert type(model[0]).__name__ == "ControlPretrainLDM"
    _linearity(model, _inputs(), "pre-train, l2")
