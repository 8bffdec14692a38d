"""Gradient clipping and norm tracking, the parts that need no GPU: the Trainer's arguments on a plain torch optimizer against a
hand-written loop, the scripts' flags, the C ABI's declarations and host-side refusals, and -- through the recording stand-in
for the library (tests/test_engine_launch_sequence.Recorder) -- what the engine's optimizers launch with the feature off and on."""
import ctypes
import importlib.util
import os
from types import SimpleNamespace

import pytest
import torch

from tests.util import ROOT


# ------------------------------------------------------------------------------------------------ Trainer on a torch optimizer

class _Small(torch.nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(3)
        self.net = torch.nn.Sequential(torch.nn.Linear(6, 16), torch.nn.Tanh(), torch.nn.Linear(16, 1))
        self.logs = []

    def training_step(self, batch, batch_idx):
        x, y = batch
        return ((self.net(x) - y) ** 2).mean() * 40.0          # gradients well above the threshold: clipping acts every step

    def configure_optimizers(self):
        return torch.optim.AdamW(self.parameters(), lr=1e-2)

    def log_dict(self, d):
        self.logs.append(dict(d))


def _data(n):
    g = torch.Generator().manual_seed(9)
    return [(torch.randn(5, 6, generator=g), torch.randn(5, 1, generator=g)) for _ in range(n)]


def _hand_loop(steps, acc, max_norm):
    m = _Small().train()
    opt = m.configure_optimizers()
    norms = []
    opt.zero_grad()
    for i, batch in enumerate(_data(steps * acc)):
        (m.training_step(batch, i) / acc).backward()
        if (i + 1) % acc == 0:
            norms.append(float(torch.nn.utils.clip_grad_norm_(list(m.parameters()), max_norm)))
            opt.step()
            opt.zero_grad()
    return m, norms


@pytest.mark.parametrize("acc", [1, 2])
def test_trainer_clips_like_a_hand_written_loop(acc, tmp_path):
    from ctrlora_amd.trainer import Trainer
    want, norms = _hand_loop(4, acc, 0.5)
    assert all(n > 0.5 for n in norms), f"clipping must act on every step: {norms}"
    m = _Small()
    tr = Trainer(max_steps=4, accumulate_grad_batches=acc, device="cpu", default_root_dir=str(tmp_path), log_every_n_steps=1,
                 gradient_clip_val=0.5)
    tr.fit(m, _data(4 * acc))
    assert tr.global_step == 4
    for (k, a), (_, b) in zip(m.state_dict().items(), want.state_dict().items()):
        assert torch.equal(a, b), k
    assert tr.logged_grad_norm == list(zip((1, 2, 3, 4), norms))
    assert [d["train/grad_norm"] for d in m.logs] == norms
    # and it is not the unclipped trajectory
    free, _ = _hand_loop(4, acc, float("inf"))
    assert not all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), free.state_dict().values()))


def test_tracking_alone_measures_and_does_not_clip(tmp_path):
    from ctrlora_amd.trainer import Trainer
    want, norms = _hand_loop(4, 1, float("inf"))
    m = _Small()
    tr = Trainer(max_steps=4, device="cpu", default_root_dir=str(tmp_path), log_every_n_steps=2, track_grad_norm=2)
    tr.fit(m, _data(4))
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), want.state_dict().values()))
    assert tr.logged_grad_norm == [(2, norms[1]), (4, norms[3])], "read at log_every_n_steps only"


def test_off_by_default_and_zero_is_off(tmp_path, monkeypatch):
    from ctrlora_amd.trainer import Trainer
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", lambda *a, **k: pytest.fail("clipped with the feature off"))
    for kw in ({}, dict(gradient_clip_val=0), dict(gradient_clip_val=None, track_grad_norm=-1)):
        m = _Small()
        tr = Trainer(max_steps=3, device="cpu", default_root_dir=str(tmp_path), log_every_n_steps=1, **kw)
        tr.fit(m, _data(3))
        assert tr.logged_grad_norm == [] and m.logs == [] and tr.gradient_clip_val == 0.0 and not tr.track_grad_norm


def test_refused_arguments():
    from ctrlora_amd.trainer import Trainer
    with pytest.raises(ValueError, match="value"):
        Trainer(device="cpu", gradient_clip_val=0.5, gradient_clip_algorithm="value")
    with pytest.raises(ValueError, match="track_grad_norm"):
        Trainer(device="cpu", track_grad_norm=1)
    with pytest.raises(ValueError, match="track_grad_norm"):
        Trainer(device="cpu", track_grad_norm="inf")
    with pytest.raises(ValueError, match="gradient_clip_val"):
        Trainer(device="cpu", gradient_clip_val=-1.0)
    assert Trainer(device="cpu", gradient_clip_algorithm="norm", track_grad_norm=2).track_grad_norm


# ------------------------------------------------------------------------------------------------ scripts

def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("script", ["train_ctrlora_finetune", "train_ctrlora_pretrain"])
def test_scripts_parse_the_flags_with_their_defaults_off(script):
    p = _load(script).get_parser()
    base = ["--dataroot", "d", "--config", "c", "--sd_ckpt", "s", "--cn_ckpt", "n"]
    a = p.parse_args(base)
    assert a.grad_clip == 0.0 and a.track_grad_norm is False
    a = p.parse_args(base + ["--grad_clip", "1.5", "--track_grad_norm", "--gradacc", "2"])
    assert a.grad_clip == 1.5 and a.track_grad_norm is True and a.gradacc == 2
    if script == "train_ctrlora_finetune":
        a = p.parse_args(base + ["--grad_clip", "1.0", "--graph", "--latent_cache", "x"])
        assert a.graph and a.grad_clip == 1.0 and a.latent_cache == "x"


# ------------------------------------------------------------------------------------------------ C ABI

def test_symbols_are_declared_with_the_signatures_hip_binds():
    from ctrlora_amd import hip
    from tests.test_capi_symbols import _cls, _header_decls
    decls = _header_decls()
    P, L, I = ctypes.c_void_p, ctypes.c_long, ctypes.c_int
    want = {"cl_grad_norm_scratch_floats": ("long", [I]), "cl_grad_norm": ("int", [P, P, I, P, P, P, P, P]),
            "cl_adamw_dev_clip": ("int", [P, P, P, P, L, P, P, P, P])}
    cmap = {P: "ptr", L: "long", I: "int"}
    for name, (ret, sig) in want.items():
        assert name in decls and name in hip.EXPORTED, name
        assert decls[name][0] == ret and hip._SIGS[name] == sig
        assert [_cls(a) for a in decls[name][1]] == [cmap[s] for s in sig], name
    hdr = open(os.path.join(ROOT, "include", "ctrlora_hip.h")).read()
    assert "#define CL_ABI_VERSION 7" in hdr
    doc = hdr[:hdr.index("long cl_grad_norm_scratch_floats")]
    assert "added in ABI 7 (compatible)" in doc[doc.rindex("/*"):], "the additions are marked compatible where they are declared"
    ew = open(os.path.join(ROOT, "ctrlora_amd", "csrc", "elementwise.h")).read()
    assert "EW_QSAMPLE_BLEND, EW_GRAD_NORM, EW_ADAMW_DEV_CLIP" in ew.replace("\n", " "), "new records are appended, none renumbered"


def test_host_side_refusals_launch_nothing():
    """CL_EINVAL (1) with host addresses and no GPU: every refusal is decided before anything is launched."""
    from ctrlora_amd import hip
    L = hip.lib()
    assert L.cl_abi_version() == 7
    assert [L.cl_grad_norm_scratch_floats(n) for n in (0, 17, -1)] == [0, 0, 0]
    floats = L.cl_grad_norm_scratch_floats(1)
    assert floats > 0 and all(L.cl_grad_norm_scratch_floats(n) == floats for n in (3, 16))
    mem = (ctypes.c_float * 64)()
    p = ctypes.addressof(mem)
    N = None
    bufs = lambda *a: (ctypes.c_void_p * 17)(*a)
    cnt = lambda *a: (ctypes.c_long * 17)(*a)
    calls = {
        "nbuf=0": L.cl_grad_norm(bufs(p), cnt(4), 0, p, p, p, p, N), "nbuf=17": L.cl_grad_norm(bufs(*[p] * 17), cnt(*[1] * 17), 17, p, p, p, p, N),
        "count<0": L.cl_grad_norm(bufs(p, p), cnt(4, -1), 2, p, p, p, p, N), "null out": L.cl_grad_norm(bufs(p), cnt(4), 1, p, p, N, p, N),
        "null scratch": L.cl_grad_norm(bufs(p), cnt(4), 1, p, p, p, N, N), "null hyper": L.cl_grad_norm(bufs(p), cnt(4), 1, N, p, p, p, N),
        "null buffer, count>0": L.cl_grad_norm(bufs(p, None), cnt(4, 4), 2, p, p, p, p, N),
        "null bufs": L.cl_grad_norm(N, cnt(4), 1, p, p, p, p, N), "null counts": L.cl_grad_norm(bufs(p), N, 1, p, p, p, p, N),
        "buffer off 4 bytes": L.cl_grad_norm(bufs(p + 2), cnt(4), 1, p, p, p, p, N), "scratch off 8 bytes": L.cl_grad_norm(bufs(p), cnt(4), 1, p, p, p, p + 4, N),
        "clip null": L.cl_adamw_dev_clip(p, p, p, p, 1, p, p, N, N), "clip n<0": L.cl_adamw_dev_clip(p, p, p, p, -1, p, p, p, N),
        "clip null hyper": L.cl_adamw_dev_clip(p, p, p, p, 0, N, p, p, N), "clip null g": L.cl_adamw_dev_clip(p, N, p, p, 1, p, p, p, N),
    }
    wrong = {k: v for k, v in calls.items() if v != 1}
    assert not wrong, wrong
    out = (ctypes.c_int * 8)(*([7] * 8))
    assert L.cl_debug_ew_last_launch(out) == 0 and list(out) == [0] * 8
    assert all(v == 0.0 for v in mem)


# ------------------------------------------------------------------------------------------------ what the optimizers launch

def _fake_ex(n, seed):
    g = torch.Generator().manual_seed(seed)
    tr = SimpleNamespace(flat=torch.randn(n, generator=g), flat_grad=torch.randn(n, generator=g), items=[], by_name={})
    return SimpleNamespace(tr=tr, repack=lambda: None)


@pytest.fixture
def rec(monkeypatch):
    from ctrlora_amd import hip
    from tests.test_engine_launch_sequence import Recorder
    r = Recorder({})
    monkeypatch.setattr(hip, "_lib", r)
    monkeypatch.setattr(hip, "stream", lambda: 0)
    return r


def test_fused_adamw_launches(rec):
    from ctrlora_amd.train import FusedAdamW
    exs = [_fake_ex(40, 1), _fake_ex(24, 2)]
    opt = FusedAdamW([torch.nn.Parameter(ex.tr.flat) for ex in exs], exs, lr=1e-3)
    assert opt.max_grad_norm is None and opt.track_grad_norm is False and not opt.norm_enabled
    assert opt.grad_norm_out.tolist() == [0.0, 1.0] and opt._max_norm.tolist() == [0.0]
    norm, coef = opt.last_grad_norm()
    assert norm.data_ptr() == opt.grad_norm_out.data_ptr() and coef.data_ptr() == opt.grad_norm_out.data_ptr() + 4
    opt.step()
    today = [("cl_tick", 2), ("cl_adamw_dev", 8), ("cl_adamw_dev", 8)]
    assert [(n, len(a)) for n, a in rec.calls] == today, "the default path launches exactly what it did"
    for (_, a), ex, st in zip(rec.calls[1:], exs, opt._states):
        assert a[:7] == (ex.tr.flat.data_ptr(), ex.tr.flat_grad.data_ptr(), st.m.data_ptr(), st.v.data_ptr(), ex.tr.flat.numel(),
                         opt._hyper.data_ptr(), opt._step_dev.data_ptr())
    for setting in (dict(max_grad_norm=0.0), dict(max_grad_norm=None, track_grad_norm=False)):
        rec.clear()
        for k, v in setting.items():
            setattr(opt, k, v)
        opt.step()
        assert [(n, len(a)) for n, a in rec.calls] == today, setting

    for setting, threshold in ((dict(max_grad_norm=2.5), 2.5), (dict(max_grad_norm=None, track_grad_norm=True), 0.0),
                               (dict(max_grad_norm=0.75, track_grad_norm=True), 0.75)):
        rec.clear()
        for k, v in setting.items():
            setattr(opt, k, v)
        opt.step()
        assert rec.names() == ["cl_grad_norm_scratch_floats"] * (setting == dict(max_grad_norm=2.5)) + \
            ["cl_grad_norm", "cl_tick", "cl_adamw_dev_clip", "cl_adamw_dev_clip"], (setting, rec.names())
        assert opt._max_norm.tolist() == [threshold], "sync_hyper() refreshes the threshold with the hyper-parameters"
        (gn,) = rec.of("cl_grad_norm")
        assert [gn[0][i] for i in range(2)] == [ex.tr.flat_grad.data_ptr() for ex in exs] and list(gn[1])[:2] == [40, 24]
        assert gn[2:7] == (2, opt._hyper.data_ptr(), opt._max_norm.data_ptr(), opt.grad_norm_out.data_ptr(), opt._norm_scratch.data_ptr())
        for a, ex, st in zip(rec.of("cl_adamw_dev_clip"), exs, opt._states):
            assert a[:8] == (ex.tr.flat.data_ptr(), ex.tr.flat_grad.data_ptr(), st.m.data_ptr(), st.v.data_ptr(), ex.tr.flat.numel(),
                             opt._hyper.data_ptr(), opt._step_dev.data_ptr(), opt.grad_norm_out.data_ptr())


def test_pretrain_adamw_norm_covers_base_and_active_banks(rec):
    from ctrlora_amd.train import PretrainAdamW
    base = _fake_ex(64, 1)
    banks = {t: _fake_ex(32, 10 + i).tr for i, t in enumerate(("hed", "canny", "depth"))}
    opt = PretrainAdamW([torch.nn.Parameter(base.tr.flat)], base, banks, lr=1e-3)
    opt.mark_used("canny")
    opt.step()
    assert rec.names() == ["cl_tick", "cl_adamw_dev"] * 2, "the default path launches exactly what it did"
    opt.max_grad_norm = 1.0
    for active in (["canny"], ["canny", "hed"]):
        opt.mark_used(active[-1])
        rec.clear()
        opt.step()
        names = [n for n in rec.names() if n != "cl_grad_norm_scratch_floats"]
        assert names == ["cl_grad_norm"] + ["cl_tick", "cl_adamw_dev_clip"] * (1 + len(active))
        (gn,) = rec.of("cl_grad_norm")
        want = [base.tr.flat_grad] + [banks[t].flat_grad for t in active]        # an idle active bank: its zero gradient
        assert gn[2] == len(want) and [gn[0][i] for i in range(gn[2])] == [w.data_ptr() for w in want]
        assert list(gn[1])[:gn[2]] == [w.numel() for w in want]


def test_more_than_sixteen_buffers_are_refused_in_python(rec):
    from ctrlora_amd.train import FusedAdamW
    exs = [_fake_ex(8, i) for i in range(17)]
    opt = FusedAdamW([torch.nn.Parameter(ex.tr.flat) for ex in exs], exs)
    opt.track_grad_norm = True
    with pytest.raises(ValueError, match="at most 16"):
        opt.step()
    assert "cl_tick" not in rec.names(), "refused before anything of the step was launched"
