"""Learning-rate schedules on the host: WarmupDecay's closed forms, compile_lambda_lr against a real LambdaLR, the Trainer's
handling of what configure_optimizers() may return (stepping, accumulation, checkpoint, resume, refusals) with a plain torch AdamW on
the CPU, and the script's flags.  No GPU."""
import importlib.util
import math
import os

import pytest
import torch

from tests.util import ROOT


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------ WarmupDecay

def test_warmup_decay_closed_forms_at_the_corners():
    from ctrlora_amd.lr_schedule import WarmupDecay
    W, T = 4, 20
    for kind in ("constant", "linear", "cosine"):
        for mr in (0.0, 0.25, 1.0):
            s = WarmupDecay(kind, W, T, mr).schedule
            assert s(0) == 1 / W and s(W - 1) == 1.0 and s(1) == 2 / W, (kind, mr)
            assert s(W) == 1.0, "q = 0: the decay starts at the full rate"
            end = 1.0 if kind == "constant" else mr
            assert s(T) == pytest.approx(end, abs=1e-15) and s(T + 1) == s(T) == s(10 * T), "flat beyond total_steps"
            mid = (W + T) // 2
            q = (mid - W) / (T - W)
            want = {"constant": 1.0, "linear": 1 - (1 - mr) * q, "cosine": mr + (1 - mr) * 0.5 * (1 + math.cos(math.pi * q))}[kind]
            assert s(mid) == want and isinstance(s(mid), float)
            if mr == 1.0:
                assert all(s(n) == pytest.approx(1.0, abs=1e-15) for n in range(W, 3 * T)), "min_ratio 1: no decay at all"
    # no warm-up: the first step is on the curve already
    for kind in ("constant", "linear", "cosine"):
        s = WarmupDecay(kind, 0, 10).schedule
        assert s(0) == 1.0 and s(10) == (1.0 if kind == "constant" else pytest.approx(0.0, abs=1e-15))
    assert WarmupDecay("linear", 0, 10).schedule(5) == 0.5
    # warm-up as long as the run, or longer: max(1, ...) keeps q finite
    s = WarmupDecay("cosine", 10, 10, 0.1).schedule
    assert s(9) == 1.0 and s(10) == 1.0 and s(11) == pytest.approx(0.1)
    assert WarmupDecay("linear", 30, 10).schedule(29) == 1.0


@pytest.mark.parametrize("bad", [dict(kind="poly"), dict(warmup_steps=-1), dict(warmup_steps=1.5), dict(total_steps=0), dict(min_ratio=-0.1),
                                 dict(min_ratio=1.01), dict(min_ratio=float("nan"))])
def test_warmup_decay_refuses_bad_arguments(bad):
    from ctrlora_amd.lr_schedule import WarmupDecay
    args = dict(kind="cosine", warmup_steps=2, total_steps=10, min_ratio=0.0)
    args.update(bad)
    with pytest.raises(ValueError):
        WarmupDecay(**args)


# ------------------------------------------------------------------------------------------------ compile_lambda_lr

def test_compiled_table_is_the_fp32_of_a_real_lambda_lr_trajectory():
    from torch.optim.lr_scheduler import LambdaLR, StepLR
    from ctrlora_amd.lr_schedule import WarmupDecay, compile_lambda_lr
    T = 37
    a, b = torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2))
    mk = lambda: torch.optim.AdamW([dict(params=[a], lr=1e-5), dict(params=[b], lr=4e-5 / 3)])
    lams = [WarmupDecay("cosine", 5, 30, 0.1).schedule, lambda n: 0.97 ** n]
    table = compile_lambda_lr(LambdaLR(mk(), lr_lambda=lams), T)
    assert table.dtype == torch.float32 and tuple(table.shape) == (T, 2)
    opt = mk()
    sched = LambdaLR(opt, lr_lambda=lams)
    for n in range(T):
        want = torch.tensor([g["lr"] for g in opt.param_groups], dtype=torch.float64).to(torch.float32)
        assert torch.equal(table[n], want), (n, table[n].tolist(), want.tolist())
        a.grad, b.grad = torch.ones(3), torch.ones(2)
        opt.step()
        sched.step()
    # one lambda for every group, and a table that does not move the scheduler it was compiled from
    opt = mk()
    sched = LambdaLR(opt, lr_lambda=lams[0])
    t2 = compile_lambda_lr(sched, 4)
    assert sched.last_epoch == 0 and torch.equal(t2[:, 0], table[:4, 0]) and t2[0, 1] == torch.tensor(4e-5 / 3 / 5, dtype=torch.float64).float()
    with pytest.raises(TypeError, match="LambdaLR"):
        compile_lambda_lr(StepLR(mk(), 3), 4)
    with pytest.raises(ValueError):
        compile_lambda_lr(sched, 0)


# ------------------------------------------------------------------------------------------------ the Trainer, on the CPU

class _Small(torch.nn.Module):
    """A two-layer regression with the hooks the Trainer calls; `form` picks what configure_optimizers() returns."""

    def __init__(self, form="tuple_dict", lam=None, interval="step", sched_cls=None):
        super().__init__()
        torch.manual_seed(3)
        self.net = torch.nn.Sequential(torch.nn.Linear(4, 8), torch.nn.Tanh(), torch.nn.Linear(8, 2))
        self.form, self.lam, self.interval, self.sched_cls = form, lam, interval, sched_cls
        self.logs = []

    def training_step(self, batch, batch_idx):
        x, y = batch
        return ((self.net(x) - y) ** 2).mean()

    def log_dict(self, d):
        self.last_logged = dict(d)
        self.logs.append(dict(d))

    def configure_optimizers(self):
        from torch.optim.lr_scheduler import LambdaLR
        opt = torch.optim.AdamW(self.net.parameters(), lr=1e-2)
        if self.form == "bare":
            return opt
        if self.form == "list":
            return [opt]
        sched = self.sched_cls(opt) if self.sched_cls else LambdaLR(opt, lr_lambda=self.lam)
        if self.form == "tuple_bare":
            return [opt], [sched]
        entry = {"scheduler": sched, "interval": self.interval, "frequency": 1}
        if self.form == "tuple_dict":
            return [opt], [entry]
        if self.form == "dict":
            return {"optimizer": opt, "lr_scheduler": entry}
        if self.form == "dict_bare":
            return {"optimizer": opt, "lr_scheduler": sched}
        raise AssertionError(self.form)


def _data(n):
    g = torch.Generator().manual_seed(9)
    return [(torch.randn(5, 4, generator=g), torch.randn(5, 2, generator=g)) for _ in range(n)]


def _lam():
    from ctrlora_amd.lr_schedule import WarmupDecay
    return WarmupDecay("cosine", 2, 6, 0.1).schedule


def _trainer(tmp_path, steps, acc=1, callbacks=()):
    from ctrlora_amd.trainer import Trainer
    return Trainer(max_steps=steps, accumulate_grad_batches=acc, device="cpu", default_root_dir=str(tmp_path), log_every_n_steps=1,
                   callbacks=list(callbacks))


class _LrProbe:
    """The optimizer's lr after every micro-batch (after the scheduler moved, where it did)."""

    def __init__(self):
        self.seen = []

    def on_train_batch_end(self, trainer, module, outputs, batch, batch_idx):
        self.seen.append((trainer.global_step, trainer.optimizer.param_groups[0]["lr"]))


@pytest.mark.parametrize("form", ["bare", "list", "tuple_bare", "tuple_dict", "dict", "dict_bare"])
def test_every_return_form_of_configure_optimizers(form, tmp_path):
    lam = _lam()
    m = _Small(form, lam)
    probe = _LrProbe()
    tr = _trainer(tmp_path, 6, callbacks=[probe]).fit(m, _data(6))
    assert tr.global_step == 6 and isinstance(tr.optimizer, torch.optim.AdamW)
    if form in ("bare", "list"):
        assert tr.lr_scheduler is None and tr.logged_lr == [] and [lr for _, lr in probe.seen] == [1e-2] * 6
        assert not any("train/lr" in d for d in m.logs)
        return
    # the lr moved: after optimizer step s the next step's rate, lambda(s), is in place; step s itself used lambda(s - 1)
    assert [lr for _, lr in probe.seen] == [1e-2 * lam(s) for s in range(1, 7)], "on the parent commit the lr never moves"
    assert tr.logged_lr == [(s, {"train/lr": 1e-2 * lam(s - 1)}) for s in range(1, 7)]
    assert [d["train/lr"] for d in m.logs if "train/lr" in d] == [1e-2 * lam(s - 1) for s in range(1, 7)]
    assert tr.lr_scheduler.last_epoch == 6


def test_scheduler_steps_once_per_optimizer_step_under_accumulation(tmp_path):
    lam = _lam()
    probe = _LrProbe()
    tr = _trainer(tmp_path, 4, acc=3, callbacks=[probe]).fit(_Small("tuple_dict", lam), _data(12))
    assert tr.global_step == 4 and tr.lr_scheduler.last_epoch == 4, "12 micro-batches, 4 scheduler steps"
    assert probe.seen == [(s, 1e-2 * lam(s)) for s in (0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4)]
    # and the weights are those of stepping by hand with the same rule
    ref = _Small("bare")
    opt = torch.optim.AdamW(ref.net.parameters(), lr=1e-2)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lam)
    for i, b in enumerate(_data(12)):
        (ref.training_step(b, i) / 3).backward()
        if i % 3 == 2:
            opt.step()
            opt.zero_grad()
            sched.step()
    got = tr.model.net.state_dict()
    assert all(torch.equal(got[k], v) for k, v in ref.net.state_dict().items())


def test_checkpoint_carries_the_scheduler_and_a_resume_continues_the_curve(tmp_path):
    lam = _lam()
    data = _data(6)
    whole = _trainer(tmp_path / "whole", 6).fit(_Small("tuple_dict", lam), data)
    a = _trainer(tmp_path / "a", 3).fit(_Small("tuple_dict", lam), data[:3])
    ck = str(tmp_path / "three.ckpt")
    a.save_checkpoint(ck)
    saved = torch.load(ck, map_location="cpu", weights_only=False)
    assert sorted(saved) == ["epoch", "global_step", "lr_schedulers", "optimizer_states", "state_dict"]
    assert len(saved["lr_schedulers"]) == 1 and saved["lr_schedulers"][0]["last_epoch"] == 3
    probe = _LrProbe()
    b = _trainer(tmp_path / "b", 6, callbacks=[probe]).fit(_Small("tuple_dict", lam), data[3:], ckpt_path=ck)
    assert b.global_step == 6 and b.lr_scheduler.last_epoch == 6
    assert [lr for _, lr in probe.seen] == [1e-2 * lam(s) for s in (4, 5, 6)]
    assert b.logged_lr == whole.logged_lr[3:], "steps 4..6 use the rates the uninterrupted run used"
    w, g = whole.model.net.state_dict(), b.model.net.state_dict()
    assert all(torch.equal(w[k], g[k]) for k in w)
    # a checkpoint without a scheduler has no such key (what the existing checkpoints look like)
    plain = _trainer(tmp_path / "p", 1).fit(_Small("bare"), data[:1])
    plain.save_checkpoint(str(tmp_path / "plain.ckpt"))
    assert "lr_schedulers" not in torch.load(str(tmp_path / "plain.ckpt"), map_location="cpu", weights_only=False)


def test_refusals(tmp_path):
    from ctrlora_amd.trainer import Trainer
    with pytest.raises(ValueError, match="interval='epoch'.*once per optimizer step"):
        _trainer(tmp_path, 2).fit(_Small("tuple_dict", _lam(), interval="epoch"), _data(2))
    opt = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda n: 1.0)
    with pytest.raises(ValueError, match="2 optimizers"):
        Trainer.unpack_optimizers([opt, opt])
    with pytest.raises(ValueError, match="2 schedulers"):
        Trainer.unpack_optimizers(([opt], [sched, sched]))
    assert Trainer.unpack_optimizers(([opt], [])) == (opt, None)
    assert Trainer.unpack_optimizers({"optimizer": opt}) == (opt, None)
    assert Trainer.unpack_optimizers((opt,)) == (opt, None)


def test_any_scheduler_class_is_stepped_on_a_plain_optimizer(tmp_path):
    from functools import partial
    from torch.optim.lr_scheduler import StepLR
    probe = _LrProbe()
    _trainer(tmp_path, 4, callbacks=[probe]).fit(_Small("tuple_bare", sched_cls=partial(StepLR, step_size=2, gamma=0.5)), _data(4))
    assert [lr for _, lr in probe.seen] == [1e-2, 5e-3, 5e-3, 2.5e-3]


# ------------------------------------------------------------------------------------------------ the script's flags

BASE = ["--dataroot", "d", "--config", "c", "--sd_ckpt", "k", "--cn_ckpt", "k"]


def test_flags_are_off_by_default_and_reach_the_model_config():
    ft = _script("train_ctrlora_finetune")
    p = ft.get_parser()
    a = p.parse_args(BASE)
    assert (a.lr_schedule, a.lr_warmup_steps, a.lr_min_ratio, a.lora_plus_ratio, a.no_decay_norm_bias) == (None, 0, 0.0, None, False)
    assert ft.lr_model_params(a.max_steps, a.lr_schedule, a.lr_warmup_steps, a.lr_min_ratio, a.lora_plus_ratio, a.no_decay_norm_bias) == {}
    a = p.parse_args(BASE + ["--max_steps", "500", "--lr_schedule", "cosine", "--lr_warmup_steps", "20", "--lr_min_ratio", "0.1",
                             "--lora_plus_ratio", "16", "--no_decay_norm_bias"])
    got = ft.lr_model_params(a.max_steps, a.lr_schedule, a.lr_warmup_steps, a.lr_min_ratio, a.lora_plus_ratio, a.no_decay_norm_bias)
    assert got == {"scheduler_config": {"target": "ctrlora_amd.lr_schedule.WarmupDecay",
                                        "params": {"kind": "cosine", "warmup_steps": 20, "total_steps": 500, "min_ratio": 0.1}},
                   "optim_groups": [{"name": "lora_up", "match": ["lora_layer.up."], "lr_scale": 16.0},
                                    {"name": "no_decay", "match": ["norm", ".bias"], "weight_decay": 0.0}]}
    from ldm.util import instantiate_from_config
    s = instantiate_from_config(got["scheduler_config"])
    assert (s.kind, s.warmup_steps, s.total_steps, s.min_ratio) == ("cosine", 20, 500, 0.1)
    # each flag alone
    assert list(ft.lr_model_params(10, lora_plus_ratio=4.0)) == ["optim_groups"]
    assert ft.lr_model_params(10, no_decay_norm_bias=True)["optim_groups"] == [{"name": "no_decay", "match": ["norm", ".bias"], "weight_decay": 0.0}]
    assert ft.lr_model_params(10, lr_warmup_steps=3)["scheduler_config"]["params"]["kind"] == "constant"


@pytest.mark.parametrize("bad", [["--lora_plus_ratio", "0"], ["--lora_plus_ratio", "-2"], ["--lora_plus_ratio", "nan"], ["--lr_warmup_steps", "-1"],
                                 ["--lr_min_ratio", "-0.1"], ["--lr_min_ratio", "1.5"], ["--lr_schedule", "poly"]])
def test_argparse_refuses_bad_values(bad, capsys):
    ft = _script("train_ctrlora_finetune")
    with pytest.raises(SystemExit):
        ft.get_parser().parse_args(BASE + bad)
    assert bad[0] in capsys.readouterr().err
