"""ctrlora_amd.train without a GPU: the capture plan of GraphedTrainStep, and what FusedAdamW / PretrainAdamW write to and
read from a checkpoint -- round trips by parameter name, both legacy flat formats, and refusals that must leave the optimizer
untouched.  FusedAdamW runs on oracle.arch.TINY's layout_only executor, PretrainAdamW on test_parallel_gloo's fake control model
with its CPU stand-ins for the three kernels."""
import copy
from types import SimpleNamespace

import pytest
import torch

from ctrlora_amd import hip
from ctrlora_amd.train import FusedAdamW, PretrainAdamW
from oracle import arch
from tests.flags_common import netcfg
from tests.test_parallel_gloo import _FakePretrainCN, _cpu_kernels


# ------------------------------------------------------------------ the capture plan

def test_capture_plan_is_the_documented_table():
    from ctrlora_amd.train import Piece, capture_plan
    Z, B = Piece("Z"), Piece("B")
    F = lambda **kw: Piece("F", **kw)
    table = {
        ("one", False): [F(segmented=False, tag=None, zero=True, with_opt=True)],
        ("two", False): [F(segmented=False, tag="all", zero=True, with_opt=False), B],
        ("segmented", False): [F(segmented=True, tag="per-segment", zero=True, with_opt=False), B],
        ("one", True): [Z, F(segmented=False, tag=None, zero=False, with_opt=False), B],
        ("two", True): [Z, F(segmented=False, tag="all", zero=False, with_opt=False), B],
        ("segmented", True): [Z, F(segmented=True, tag="per-segment", zero=False, with_opt=False), B],
    }
    for (mode, accumulate), want in table.items():
        assert capture_plan(mode, accumulate) == want, (mode, accumulate)
    assert Z == Piece("Z", segmented=False, tag=None, zero=False, with_opt=False)       # the defaults the table leans on
    assert B == Piece("B", segmented=False, tag=None, zero=False, with_opt=False)


# ------------------------------------------------------------------ FusedAdamW

def _fused(dtype=torch.float32, seed=1, **kw):
    sd = arch.make_state(arch.controlnet_shapes(arch.TINY), seed)
    ex = _executor(sd, dtype)
    return FusedAdamW([torch.nn.Parameter(ex.tr.flat)], [ex], **kw), ex


def _executor(sd, dtype):
    from ctrlora_amd.engine import ControlNetE
    return ControlNetE(sd, netcfg(arch.TINY), dtype, torch.device("cpu"), layout_only=True)


def _fill_distinct(opt):
    n = opt._m[0].numel()
    opt._m[0].copy_(torch.arange(n, dtype=torch.float32) + 0.25)
    opt._v[0].copy_(torch.arange(n, dtype=torch.float32) * 2 + 0.5)


def _assert_by_name(opt, ex, m, v):
    for t in ex.tr.items:
        k = t.master.numel()
        assert torch.equal(opt._m[0][t.offset:t.offset + k], m[t.name].reshape(-1)), t.name
        assert torch.equal(opt._v[0][t.offset:t.offset + k], v[t.name].reshape(-1)), t.name


def test_fused_adamw_round_trip_by_name():
    opt, ex = _fused(lr=1e-3)
    _fill_distinct(opt)
    opt._step_dev.fill_(11)
    opt.param_groups[0]["lr"] = 3e-5             # a scheduler moved it before the save
    sd = opt.state_dict()
    assert set(sd) == {"step", "format", "m", "v", "param_groups"} and sd["format"] == "by_name" and sd["step"] == 11
    assert len(sd["m"]) == len(sd["v"]) == 1 and set(sd["m"][0]) == set(sd["v"][0]) == {t.name for t in ex.tr.items}
    assert all("params" not in g for g in sd["param_groups"])
    new, ex2 = _fused(lr=1e-3)
    new.load_state_dict(sd)
    _assert_by_name(new, ex2, sd["m"][0], sd["v"][0])
    _assert_by_name(new, ex2, *[{t.name: buf[t.offset:t.offset + t.master.numel()] for t in ex.tr.items} for buf in (opt._m[0], opt._v[0])])
    assert new._step == 11
    g = new.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"]) == (3e-5, (0.9, 0.999), 1e-8, 1e-2)
    assert new._hyper[0].item() == pytest.approx(3e-5)          # ... and went to the device tensor


def _legacy_flat(ex, buf):
    """The rounds 1-3 file layout of one moment: `legacy_item_names` order, every tensor padded to 64 floats."""
    by_name = {t.name: t for t in ex.tr.items}
    names = getattr(ex, "legacy_item_names", None) or [t.name for t in ex.tr.items]
    parts = []
    for n in names:
        t = by_name[n]
        k = t.master.numel()
        parts += [buf[t.offset:t.offset + k], torch.zeros(-k % 64)]
    return torch.cat(parts)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_adamw_loads_the_legacy_flat_format(dtype):
    """bf16 hoists the grouped emb_layers factors to the tail of the flat buffer, so the legacy order differs from today's."""
    opt, ex = _fused(dtype)
    _fill_distinct(opt)
    want = opt.state_dict()
    legacy = dict(step=9, m=[_legacy_flat(ex, opt._m[0])], v=[_legacy_flat(ex, opt._v[0])], param_groups=want["param_groups"])
    new, ex2 = _fused(dtype)
    new.load_state_dict(legacy)
    _assert_by_name(new, ex2, want["m"][0], want["v"][0])
    assert new._step == 9
    # 64 floats short: refused, nothing changed -- not m (whose tensor is fine), not v, not the counter
    new._m[0].fill_(3.0); new._v[0].fill_(4.0); new._step_dev.fill_(2)
    short = dict(legacy, v=[legacy["v"][0][:-64].clone()])
    with pytest.raises(ValueError, match="legacy optimizer state holds"):
        new.load_state_dict(short)
    assert bool((new._m[0] == 3.0).all()) and bool((new._v[0] == 4.0).all()) and new._step == 2


# ------------------------------------------------------------------ PretrainAdamW

_SIZES = {64: (10, 20, 24), 32: (5, 11, 8)}       # tensors at 0 / 16 / 40 resp. 0 / 8 / 24: gaps, as the 64-float padding leaves


def _named(ts, prefix):
    """Give a fake flat set the `items` / `by_name` of a TrainableSet."""
    sizes = _SIZES[ts.numel]
    offs = (0, 16, 40) if ts.numel == 64 else (0, 8, 24)
    ts.items = [SimpleNamespace(name=f"{prefix}.{i}", offset=o, master=ts.flat[o:o + k]) for i, (o, k) in enumerate(zip(offs, sizes))]
    ts.by_name = {t.name: t for t in ts.items}
    return ts


def _pretrain(monkeypatch):
    for name in ("tick", "zero_", "adamw_dev"):
        monkeypatch.setattr(hip, name, getattr(hip, name))        # restored after the test
    _cpu_kernels(hip)
    cm = _FakePretrainCN()
    _named(cm.executor().tr, "base")
    for t in cm.tasks:
        _named(cm.bank(t), "lora")
    params = [torch.nn.Parameter(cm.executor().tr.flat)] + [torch.nn.Parameter(cm.bank(t).flat) for t in cm.tasks]
    return PretrainAdamW(params, cm.executor(), {t: cm.bank(t) for t in cm.tasks}, lr=1e-2), cm


def _states(opt):
    """[(key, flat set, its Adam state as a mapping with "m" | "v" | "step")]"""
    return [("base", opt.executor.tr, opt._base)] + [(k, ts, opt._bank_state[k]) for k, ts in opt.banks.items()]


def _two_steps(opt, cm):
    for step, task in enumerate(("hed", "depth")):
        opt.mark_used(task)
        gen = torch.Generator().manual_seed(step)
        cm.executor().tr.flat_grad += torch.randn(64, generator=gen)
        cm.bank(task).flat_grad += torch.randn(32, generator=gen)
        opt.step()
        opt.zero_grad()


def _used(ts, buf):
    return torch.cat([buf[t.offset:t.offset + t.master.numel()] for t in ts.items])


def test_pretrain_adamw_round_trip_and_format_1(monkeypatch):
    opt, cm = _pretrain(monkeypatch)
    _two_steps(opt, cm)
    opt.param_groups[0]["lr"] = 5e-4
    sd = opt.state_dict()
    assert set(sd) == {"format", "version", "base", "banks", "active", "param_groups"}
    assert (sd["format"], sd["version"], sd["active"]) == ("by_name", 2, ["hed", "depth"])
    assert set(sd["banks"]) == set(cm.tasks) and all(set(b) == {"m", "v", "step"} for b in [sd["base"], *sd["banks"].values()])
    assert [sd["base"]["step"]] + [sd["banks"][t]["step"] for t in cm.tasks] == [2, 2, 0, 1]      # hed, canny, depth
    assert float(sd["banks"]["hed"]["v"]["lora.1"].abs().sum()) > 0 and float(sd["banks"]["canny"]["v"]["lora.1"].abs().sum()) == 0

    new, cm2 = _pretrain(monkeypatch)
    new.load_state_dict(sd)
    for (k, ts, a), (_, ts2, b) in zip(_states(opt), _states(new)):
        for key in ("m", "v"):
            assert torch.equal(_used(ts, a[key]), _used(ts2, b[key])), (k, key)
        assert int(a["step"]) == int(b["step"]), k
    assert new.active == ["hed", "depth"] and new._step == 2 and new.param_groups[0]["lr"] == 5e-4

    # format 1: the raw flat buffers of equal numel
    raw = {k: dict(m=st["m"].clone(), v=st["v"].clone(), step=int(st["step"])) for k, _, st in _states(opt)}
    sd1 = dict(base=raw.pop("base"), banks=raw, active=list(opt.active), param_groups=sd["param_groups"])
    new1, _ = _pretrain(monkeypatch)
    new1.load_state_dict(sd1)
    for (k, _, a), (_, _, b) in zip(_states(opt), _states(new1)):
        assert torch.equal(a["m"], b["m"]) and torch.equal(a["v"], b["v"]) and int(a["step"]) == int(b["step"]), k
    assert new1.active == ["hed", "depth"]
    bad = copy.deepcopy(sd1)
    bad["base"]["m"] = bad["base"]["m"][:-1].clone()
    with pytest.raises(ValueError, match="does not fit this build"):
        new1.load_state_dict(bad)


@pytest.mark.parametrize("case", ["last bank lacks a tensor in v", "another bank set", "format 1 buffer of the wrong length"])
def test_pretrain_adamw_refusal_changes_nothing(monkeypatch, case):
    """A refused state dict must not leave a half-loaded optimizer: every moment, every counter and `active` stay."""
    src, cm = _pretrain(monkeypatch)
    _two_steps(src, cm)
    sd = src.state_dict()
    last = list(sd["banks"])[-1]
    if case == "last bank lacks a tensor in v":
        del sd["banks"][last]["v"]["lora.2"]
        err, match = KeyError, "optimizer state lacks"
    elif case == "another bank set":
        sd["banks"]["normal"] = sd["banks"].pop(last)
        err, match = KeyError, "optimizer state holds banks"
    else:
        sd["banks"][last]["m"] = torch.zeros(31)
        sd["banks"][last]["v"] = torch.zeros(32)
        err, match = ValueError, "does not fit this build"
    opt, _ = _pretrain(monkeypatch)
    for i, (_, _, st) in enumerate(_states(opt)):
        st["m"].fill_(100.0 + i); st["v"].fill_(200.0 + i); st["step"].fill_(40 + i)
    opt.active = ["canny"]
    with pytest.raises(err, match=match):
        opt.load_state_dict(sd)
    for i, (k, _, st) in enumerate(_states(opt)):
        assert bool((st["m"] == 100.0 + i).all()), f"{k}: a refused load overwrote m"
        assert bool((st["v"] == 200.0 + i).all()), f"{k}: a refused load overwrote v"
        assert int(st["step"]) == 40 + i, f"{k}: a refused load moved the step counter"
    assert opt.active == ["canny"] and opt.param_groups[0]["lr"] == 1e-2


# ------------------------------------------------------------------ state dicts as the previous code wrote them

def test_state_dicts_of_the_previous_layout_load(monkeypatch):
    """Both dict shapes built by hand from their key lists: {step, format, m: [{name: t}], v: [...], param_groups} and
    {format, version: 2, base: {m, v, step}, banks: {task: {m, v, step}}, active, param_groups}."""
    groups = [dict(lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)]
    opt, ex = _fused()
    gen = torch.Generator().manual_seed(3)
    mk = lambda items: {t.name: torch.randn(t.master.shape, generator=gen) for t in items}      # saved in the tensor's own shape
    sd = dict(step=5, format="by_name", m=[mk(ex.tr.items)], v=[mk(ex.tr.items)], param_groups=groups)
    opt.load_state_dict(sd)
    _assert_by_name(opt, ex, sd["m"][0], sd["v"][0])
    assert opt._step == 5 and opt.param_groups[0]["lr"] == 2e-4

    popt, cm = _pretrain(monkeypatch)
    part = lambda ts, step: dict(m=mk(ts.items), v=mk(ts.items), step=step)
    psd = dict(format="by_name", version=2, base=part(cm.executor().tr, 6),
               banks={t: part(cm.bank(t), i) for i, t in enumerate(cm.tasks)}, active=["canny", "depth"], param_groups=groups)
    psd["banks"]["hed"]["m"]["surplus.name"] = torch.zeros(3)          # PretrainAdamW accepts names it does not train
    popt.load_state_dict(psd)
    for k, ts, st in _states(popt):
        src = psd["base"] if k == "base" else psd["banks"][k]
        for t in ts.items:
            n = t.master.numel()
            assert torch.equal(st["m"][t.offset:t.offset + n], src["m"][t.name]), (k, t.name)
            assert torch.equal(st["v"][t.offset:t.offset + n], src["v"][t.name]), (k, t.name)
        assert int(st["step"]) == src["step"]
    assert popt.active == ["canny", "depth"] and popt._step == 6 and popt.param_groups[0]["lr"] == 2e-4
