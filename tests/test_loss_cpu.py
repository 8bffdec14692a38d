"""Per-timestep loss weights and the Huber loss, the parts that need no GPU: the model's keywords and state dict,
set_loss_weights, the refusals, p_losses on the CPU against hand-written expressions, the scripts' flags and graph_step_refusal."""
import importlib.util
import os

import pytest
import torch
import torch.nn.functional as F

from tests.util import ROOT

FINETUNE, PRETRAIN = "ctrlora_finetune_sd15_rank128.yaml", "ctrlora_pretrain_sd15_9tasks_rank128.yaml"


def _model(config=FINETUNE, **params):
    import bench
    return bench.build_model(config, 0, tiny=True, mutate=lambda p: p.update(params))


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def plain():
    return _model()


def test_keywords_reach_the_model_from_the_config(plain):
    assert plain.min_snr_gamma == 0.0 and plain.loss_weights is None and plain.loss_type == "l2" and plain.huber_delta == 1.0
    for config in (FINETUNE, PRETRAIN):
        m = _model(config, min_snr_gamma=5, loss_type="huber", huber_delta=0.25)
        assert m.min_snr_gamma == 5.0 and m.loss_type == "huber" and m.huber_delta == 0.25
        assert m.loss_weights.dtype == torch.float32 and m.loss_weights.shape == (m.num_timesteps,)
        assert m.loss_weights_pinned is False


def test_loss_weights_is_not_in_the_state_dict(plain):
    m = _model(min_snr_gamma=5.0)
    assert "loss_weights" in dict(m.named_buffers()) and "loss_weights" not in m.state_dict()
    assert list(m.state_dict()) == list(plain.state_dict()), "checkpoints keep their keys"
    assert not plain.load_state_dict(m.state_dict()).missing_keys


def test_set_loss_weights_copies_into_the_same_tensor():
    m = _model(min_snr_gamma=5.0)
    w0, ptr = m.loss_weights, m.loss_weights.data_ptr()
    new = torch.linspace(0.0, 2.0, m.num_timesteps, dtype=torch.float64)
    m.set_loss_weights(new)
    assert m.loss_weights is w0 and m.loss_weights.data_ptr() == ptr and torch.equal(m.loss_weights, new.float())
    m.set_loss_weights(new.tolist())
    assert m.loss_weights.data_ptr() == ptr
    m.set_loss_weights(None)
    assert m.loss_weights is None and "loss_weights" not in m.state_dict()
    m.set_loss_weights(torch.ones(m.num_timesteps))
    assert m.loss_weights.dtype == torch.float32 and m.loss_weights.device == m.betas.device
    # after a capture the table may change, its presence may not
    m.loss_weights_pinned = True
    ptr = m.loss_weights.data_ptr()
    m.set_loss_weights(new)
    assert m.loss_weights.data_ptr() == ptr and torch.equal(m.loss_weights, new.float())
    with pytest.raises(RuntimeError, match="captured training step reads the loss_weights buffer.*new capture"):
        m.set_loss_weights(None)
    off = _model()
    off.loss_weights_pinned = True
    off.set_loss_weights(None)
    with pytest.raises(RuntimeError, match="recorded without a loss_weights table.*new capture"):
        off.set_loss_weights(torch.ones(off.num_timesteps))


def test_refusals():
    for gamma in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="min_snr_gamma"):
            _model(min_snr_gamma=gamma)
    for delta in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="huber_delta"):
            _model(loss_type="huber", huber_delta=delta)
    m = _model()
    n = m.num_timesteps
    with pytest.raises(ValueError, match="shape"):
        m.set_loss_weights(torch.ones(n + 1))
    for bad in (-1.0, float("nan"), float("inf")):
        w = torch.ones(n)
        w[7] = bad
        with pytest.raises(ValueError, match="finite and non-negative"):
            m.set_loss_weights(w)
    assert m.loss_weights is None
    m.loss_type = "bogus"
    with pytest.raises(NotImplementedError, match="unknown loss type"):
        m.get_loss(torch.zeros(2), torch.zeros(2))


def _cpu_p_losses(m, seed=0):
    """p_losses on the CPU with apply_model replaced by a fixed map of x_noisy (the networks run on the GPU only): returns what it
    returned and (eps, target, t)."""
    g = torch.Generator().manual_seed(seed)
    B = 5
    z, noise = torch.randn(B, 4, 8, 8, generator=g), torch.randn(B, 4, 8, 8, generator=g)
    t = torch.tensor([0, m.num_timesteps - 1, 500, 500, 37])
    m.apply_model = lambda x_noisy, t_, cond: 1.7 * x_noisy - 0.4
    m.train()
    loss, logs = m.p_losses(z, None, t, noise=noise)
    eps = 1.7 * m.q_sample(z, t, noise) - 0.4
    return loss, logs, eps, noise, t


@pytest.mark.parametrize("loss_type", ["l2", "huber"])
@pytest.mark.parametrize("gamma", [0.0, 5.0])
def test_cpu_p_losses_against_a_hand_written_expression(loss_type, gamma):
    m = _model(min_snr_gamma=gamma, loss_type=loss_type, huber_delta=0.75, l_simple_weight=0.6)
    loss, logs, eps, target, t = _cpu_p_losses(m)
    if loss_type == "huber":
        el = F.huber_loss(eps, target, reduction="none", delta=0.75)
        d = (eps - target).abs()
        assert bool((d <= 0.75).any() and (d > 0.75).any())
        assert torch.equal(m.get_loss(eps, target, mean=False), el)
        assert torch.allclose(el, torch.where(d <= 0.75, 0.5 * d * d, 0.75 * (d - 0.375)), rtol=1e-6, atol=0)
    else:
        el = (eps - target) ** 2
    per = el.mean([1, 2, 3])
    w = m.loss_weights[t] if gamma else torch.ones_like(per)
    assert (m.loss_weights is not None) == bool(gamma)
    want = 0.6 * (w * per).mean()
    assert torch.allclose(loss, want, rtol=1e-6, atol=0)
    assert torch.allclose(logs["train/loss_simple"], per.mean(), rtol=1e-6, atol=0), "the logged loss_simple stays unweighted"
    assert torch.allclose(logs["train/loss_vlb"], (m.lvlb_weights[t] * per).mean(), rtol=1e-6, atol=0)
    if gamma:
        assert float(w[0]) < 1.0 and float(w[1]) == 1.0 and not torch.allclose(loss, 0.6 * per.mean(), rtol=1e-3)


def test_cpu_p_losses_follows_set_loss_weights():
    m = _model(l_simple_weight=1.0)
    base, _, eps, target, t = _cpu_p_losses(m)
    m.set_loss_weights(torch.ones(m.num_timesteps))
    ones, _, _, _, _ = _cpu_p_losses(m)
    assert torch.equal(ones, base), "a table of exact ones changes nothing"
    w = torch.zeros(m.num_timesteps)
    w[37] = 3.0
    m.set_loss_weights(w)
    only, _, _, _, _ = _cpu_p_losses(m)
    per = ((eps - target) ** 2).mean([1, 2, 3])
    assert torch.allclose(only, 3.0 * per[4] / 5, rtol=1e-6, atol=0)


def test_script_flags():
    for name in ("train_ctrlora_finetune", "train_ctrlora_pretrain"):
        s = _script(name)
        assert s.loss_model_params() == {} and s.loss_model_params(0.0, None, None) == {}
        assert s.loss_model_params(5.0, "huber", 0.5) == dict(min_snr_gamma=5.0, loss_type="huber", huber_delta=0.5)
        assert s.loss_model_params(0.0, "l2", None) == dict(loss_type="l2")
    ft = _script("train_ctrlora_finetune")
    base = ["--dataroot", "d", "--config", "c", "--sd_ckpt", "s", "--cn_ckpt", "n"]
    a = ft.get_parser().parse_args(base)
    assert (a.min_snr_gamma, a.loss, a.huber_delta) == (0.0, None, None)
    assert ft.loss_model_params(a.min_snr_gamma, a.loss, a.huber_delta) == {}
    a = ft.get_parser().parse_args(base + ["--min_snr_gamma", "5", "--loss", "huber", "--huber_delta", "0.5", "--graph", "--gradacc", "2"])
    assert ft.loss_model_params(a.min_snr_gamma, a.loss, a.huber_delta) == dict(min_snr_gamma=5.0, loss_type="huber", huber_delta=0.5)
    with pytest.raises(SystemExit):
        ft.get_parser().parse_args(base + ["--loss", "l1"])
    # the overrides are model keywords: they build a model
    m = _model(**ft.loss_model_params(5.0, "huber", 0.5))
    assert m.loss_type == "huber" and m.huber_delta == 0.5 and m.loss_weights is not None


def test_pretrain_parser_takes_the_flags():
    pt = _script("train_ctrlora_pretrain")
    acts = {o for a in pt.get_parser()._actions for o in a.option_strings}
    assert {"--min_snr_gamma", "--loss", "--huber_delta"} <= acts
    d = {a.dest: a.default for a in pt.get_parser()._actions}
    assert pt.loss_model_params(d["min_snr_gamma"], d["loss"], d["huber_delta"]) == {}


def test_graph_step_refusal_lets_huber_through():
    from ctrlora_amd.trainer import graph_step_refusal

    class Fine:
        loss_type, original_elbo_weight = "huber", 0.0

        def engine_train_step(self, *a):
            pass

    class L1(Fine):
        loss_type = "l1"

    class Elbo(Fine):
        original_elbo_weight = 0.5

    assert graph_step_refusal(Fine()) is None
    assert "loss_type is 'l1'" in graph_step_refusal(L1())
    assert "original_elbo_weight is 0.5" in graph_step_refusal(Elbo())
    for params in (dict(loss_type="huber"), dict(min_snr_gamma=5.0), dict()):
        assert graph_step_refusal(_model(**params)) is None
    assert "loss_type is 'l1'" in graph_step_refusal(_model(loss_type="l1"))
