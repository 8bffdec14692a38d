"""Validation by timestep band without a GPU: ValPlan, the Trainer's validation loop on the host path (a small stand-in model with
get_input / q_sample / apply_model: the engine cannot run here), best.ckpt, the refusals, that a fit with validation ends with the
bits of a fit without, and the two-rank exchange of the tables over gloo."""
import contextlib
import json
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.util import ROOT

T = 1000


# ------------------------------------------------------------------------------------------------ ValPlan

def test_grid_is_the_middle_of_every_band():
    from ctrlora_amd.validation import ValPlan, band_of, band_ranges
    p = ValPlan(1000)
    assert p.grid == [50, 150, 250, 350, 450, 550, 650, 750, 850, 950] and p.nbands == 10 and p.repeats == 1 and p.seed == 0
    assert p.labels()[0] == "t0-99" and p.labels()[-1] == "t900-999"
    for T_, nb in ((1000, 7), (1000, 64), (3, 3), (10, 4), (1000, 1)):
        q = ValPlan(T_, nb)
        assert [band_of(t, T_, nb) for t in q.grid] == list(range(nb)), (T_, nb, q.grid)
        assert all(lo <= t <= hi for t, (lo, hi) in zip(q.grid, band_ranges(T_, nb)))
    for bad in (dict(nbands=0), dict(nbands=65), dict(repeats=0)):
        with pytest.raises(ValueError):
            ValPlan(1000, **bad)
    with pytest.raises(ValueError):
        ValPlan(5, nbands=6)


def test_every_band_is_hit_equally_and_passes_rotate():
    from ctrlora_amd.validation import ValPlan, band_of
    p = ValPlan(1000, nbands=10, repeats=3)
    for r in range(3):
        t = p.timesteps(range(40), r).tolist()
        hits = [0] * 10
        for v in t:
            hits[band_of(v, 1000, 10)] += 1
        assert hits == [4] * 10
        assert t[0] == p.grid[r] and t[9] == p.grid[(9 + r) % 10]
    assert p.timesteps([3, 13, 23]).tolist() == [350] * 3 and p.timesteps([]).numel() == 0


def test_the_same_triples_on_every_call_and_for_every_split():
    from ctrlora_amd.validation import ValPlan
    p = ValPlan(1000, seed=5, repeats=2)
    state = torch.get_rng_state()
    a, b = p.noise(range(6), 0, (4, 2, 2)), p.noise(range(6), 0, (4, 2, 2))
    assert torch.equal(a, b) and a.shape == (6, 4, 2, 2)
    assert torch.equal(torch.get_rng_state(), state), "the plan draws on its own generators"
    assert not torch.equal(a, p.noise(range(6), 1, (4, 2, 2))) and not torch.equal(a, ValPlan(1000, seed=6).noise(range(6), 0, (4, 2, 2)))
    # batches of 4 + 2, and the odd samples alone (another rank has the even ones): sample j's noise is the j-th draw
    s = p.noise_stream(0, (4, 2, 2))
    assert torch.equal(torch.cat([s.take([0, 1, 2, 3]), s.take([4, 5])]), a)
    assert torch.equal(p.noise([1, 3, 5], 0, (4, 2, 2)), a[[1, 3, 5]])
    with pytest.raises(AssertionError):
        s.take([2])


def test_table_logs_mean_standard_error_and_band_keys():
    from ctrlora_amd.validation import ValPlan, accumulate_bands, new_table, table_logs
    p = ValPlan(1000, nbands=4)
    x = torch.tensor([1.0, 2.0, 3.0, 6.0])
    tab = accumulate_bands(x, torch.tensor([0, 10, 300, 999]), 1000, 4, new_table(4))
    logs = table_logs(tab, p, suffix="_ema")
    assert logs["val/loss_simple_ema"] == 3.0 and logs["val/loss_simple/t0-249_ema"] == 1.5 and logs["val/loss_simple/t750-999_ema"] == 6.0
    assert "val/loss_simple/t500-749_ema" not in logs, "an empty band logs nothing"
    assert abs(logs["val/loss_simple_se_ema"] - float(x.double().std() / 2.0)) < 1e-15
    assert set(table_logs(tab, p)) == {"val/loss_simple", "val/loss_simple_se", "val/loss_simple/t0-249", "val/loss_simple/t250-499",
                                       "val/loss_simple/t750-999"}


# ------------------------------------------------------------------------------------------------ the Trainer on the host path

class _Stub(torch.nn.Module):
    """The hooks the Trainer and a validation run on the host path use.  get_input draws a 'posterior sample' on the global CPU
    generator, as the first stage does, and training_step draws t and the noise there too: anything validation drew on it would
    show in the next training step."""
    num_timesteps, first_stage_key = T, "x"

    def __init__(self, ema=False, posterior=True):
        super().__init__()
        torch.manual_seed(3)
        self.net = torch.nn.Linear(8, 8)
        self.posterior, self.all_logged, self.last_logged = posterior, [], None
        if ema:
            from ldm.modules.ema import ModelEma
            self.model_ema = ModelEma([("net." + n, p) for n, p in self.net.named_parameters()], decay=0.5)

    @property
    def device(self):
        return self.net.weight.device

    def log_dict(self, d):
        self.last_logged = dict(d)
        self.all_logged.append(dict(d))

    def get_input(self, batch, k):
        x = batch[k].float()
        return (x + 0.05 * torch.randn(x.shape) if self.posterior else x), {"c": batch["c"]}

    def q_sample(self, x_start, t, noise):
        a = (1.0 - t.float() / T).view(-1, 1, 1, 1)
        return a.sqrt() * x_start + (1.0 - a).sqrt() * noise

    def apply_model(self, x_noisy, t, cond):
        return self.net(x_noisy.flatten(1)).view_as(x_noisy) + cond["c"].view(-1, 1, 1, 1)

    def training_step(self, batch, batch_idx):
        z, cond = self.get_input(batch, "x")
        t = torch.randint(0, T, (z.shape[0],))
        noise = torch.randn_like(z)
        loss = ((self.apply_model(self.q_sample(z, t, noise), t, cond) - noise) ** 2).mean()
        self.log_dict({"train/loss_simple": float(loss.detach())})
        return loss

    def configure_optimizers(self):
        return torch.optim.AdamW(self.net.parameters(), lr=3e-2)

    @contextlib.contextmanager
    def ema_scope(self):
        params = list(self.net.parameters())
        self.model_ema.store(params)
        self.model_ema.copy_to([("net." + n, p) for n, p in self.net.named_parameters()])
        try:
            yield
        finally:
            self.model_ema.restore(params)


def _batches(n, bs, seed):
    g = torch.Generator().manual_seed(seed)
    return [{"x": torch.randn(bs, 2, 2, 2, generator=g), "c": torch.randn(bs, generator=g)} for _ in range(n)]


def _val_batches():
    return _batches(5, 4, 77) + _batches(1, 3, 78)       # 23 samples, a ragged last batch


def _fit(tmp_path, name, model=None, steps=5, **kw):
    from ctrlora_amd.trainer import Trainer
    torch.manual_seed(0)
    m = (model or _Stub()).train()
    val = kw.pop("val", None)
    tr = Trainer(max_steps=steps, device="cpu", default_root_dir=str(tmp_path / name), log_every_n_steps=1, **kw)
    tr.fit(m, _batches(steps, 4, 11), val_dataloaders=val)
    return tr, m, torch.get_rng_state()


def test_fit_logs_the_keys_and_one_json_line_per_run(tmp_path):
    from ctrlora_amd.validation import ValPlan, accumulate_bands, new_table, table_logs
    events = []

    class _Hooks:
        def on_validation_start(self, trainer, module):
            events.append(("start", trainer.global_step, module.training))

        def on_validation_end(self, trainer, module):
            events.append(("end", trainer.global_step, module.training))

    tr, m, _ = _fit(tmp_path, "on", val=_val_batches(), val_check_interval=2, callbacks=[_Hooks()])
    assert [s for s, _ in tr.logged_val] == [2, 4, 5], "every 2 optimizer steps, and once at the end of fit"
    assert events == [(k, s, True) for s in (2, 4, 5) for k in ("start", "end")], "the module is back in train() outside a run"
    plan = ValPlan(T)
    keys = {"val/loss_simple", "val/loss_simple_se"} | {f"val/loss_simple/{lab}" for lab in plan.labels()}
    for _, logs in tr.logged_val:
        assert set(logs) == keys and all(v == v and v > 0 for v in logs.values())
    assert tr.val_tables.shape == (1, 11, 3) and tr.val_tables[0, -1, 0] == 23.0
    assert tr.val_tables[0, :10, 0].tolist() == [3.0, 3.0, 3.0] + [2.0] * 7, "sample j sits in band j % 10"
    assert any(d == tr.logged_val[-1][1] for d in m.all_logged), "through model.log_dict"
    rows = [json.loads(ln) for ln in open(os.path.join(tr.log_dir, "val_log.jsonl"))]
    assert [r["global_step"] for r in rows] == [2, 4, 5]
    for r, (_, logs) in zip(rows, tr.logged_val):
        assert {k: r[k] for k in logs} == logs
    # the last run, restated: the same triples through the model as it is now, the same fork of the generator
    from ctrlora_amd.validation import run_validation
    m.eval()
    again = run_validation(m, _val_batches(), plan, device="cpu")
    assert torch.equal(again, tr.val_tables[0]) and table_logs(again, plan) == tr.logged_val[-1][1]
    want = new_table(10)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(plan.fork_seed())
        streams, j = plan.noise_stream(0, (2, 2, 2)), 0
        for b in _val_batches():
            z, cond = m.get_input(b, "x")
            js = list(range(j, j + z.shape[0]))
            j += z.shape[0]
            t, noise = plan.timesteps(js), streams.take(js)
            per = ((m.apply_model(m.q_sample(z, t, noise), t, cond) - noise) ** 2).mean(dim=(1, 2, 3))
            accumulate_bands(per.detach(), t, T, 10, want)
    assert torch.equal(want, again)
    # limit_val_batches and another plan
    tr2, _, _ = _fit(tmp_path, "limited", val=_val_batches(), val_check_interval=5, limit_val_batches=2,
                     val_plan=ValPlan(T, nbands=4, repeats=2, seed=3))
    assert len(tr2.logged_val) == 1 and tr2.val_tables[0, -1, 0] == 16.0 and tr2.val_tables.shape == (1, 5, 3)
    assert tr2.val_tables[0, :4, 0].tolist() == [4.0] * 4


def test_validation_does_not_move_the_training_trajectory(tmp_path):
    """Bit-identical parameters, logged training losses and generator state with validation on and off."""
    on, m_on, rng_on = _fit(tmp_path, "on", val=_val_batches(), val_check_interval=2, save_best=True)
    off, m_off, rng_off = _fit(tmp_path, "off")
    assert len(on.logged_val) == 3 and not off.logged_val
    assert on.logged == off.logged and len(on.logged) == 5
    for a, b in zip(m_on.net.parameters(), m_off.net.parameters()):
        assert torch.equal(a, b)
    assert torch.equal(rng_on, rng_off)
    train_on = [d for d in m_on.all_logged if "train/loss_simple" in d]
    assert train_on == m_off.all_logged
    assert not os.path.exists(os.path.join(off.log_dir, "val_log.jsonl"))


def test_best_ckpt_is_written_on_improvement_only(tmp_path, monkeypatch):
    from ctrlora_amd.trainer import Trainer
    saved = []
    real = Trainer.save_checkpoint
    monkeypatch.setattr(Trainer, "save_checkpoint", lambda self, path: (saved.append((self.global_step, os.path.basename(path))),
                                                                        real(self, path))[1])

    class _Spoil:
        """After optimizer step 3 the weights are thrown far off: the run at step 4 is worse than the one at step 2."""

        def on_batch_end(self, trainer, module):
            if trainer.global_step == 3:
                with torch.no_grad():
                    module.net.weight.add_(3.0)

    tr, m, _ = _fit(tmp_path, "best", steps=6, val=_val_batches(), val_check_interval=2, save_best=True, callbacks=[_Spoil()])
    vals = [(s, logs["val/loss_simple"]) for s, logs in tr.logged_val]
    assert [s for s, _ in vals] == [2, 4, 6] and vals[1][1] > vals[0][1]
    best, want = float("inf"), []
    for s, v in vals:
        if v < best:
            best, want = v, want + [(s, "best.ckpt")]
    assert saved == want and (4, "best.ckpt") not in saved and tr.best_val == best
    ck = torch.load(os.path.join(tr.checkpoint_callback.dirpath, "best.ckpt"), map_location="cpu", weights_only=False)
    assert ck["global_step"] == want[-1][0]
    # without save_best nothing is written
    saved.clear()
    _fit(tmp_path, "nobest", val=_val_batches(), val_check_interval=2)
    assert saved == []


def test_val_ema_adds_the_ema_keys_and_restores_the_weights(tmp_path):
    tr, m, _ = _fit(tmp_path, "ema", model=_Stub(ema=True), val=_val_batches(), val_check_interval=2, val_ema=True, save_best=True)
    plain, m_plain, _ = _fit(tmp_path, "plain", model=_Stub(ema=True), val=_val_batches(), val_check_interval=2)
    for a, b in zip(m.net.parameters(), m_plain.net.parameters()):
        assert torch.equal(a, b), "the masters are restored bit for bit"
    assert tr.val_tables.shape == (2, 11, 3) and not torch.equal(tr.val_tables[0], tr.val_tables[1])
    assert torch.equal(tr.val_tables[0], plain.val_tables[0])
    for (_, logs), (_, logs_plain) in zip(tr.logged_val, plain.logged_val):
        assert set(logs) == set(logs_plain) | {k + "_ema" for k in logs_plain}
        assert {k: logs[k] for k in logs_plain} == logs_plain
    assert tr.best_val == min(logs["val/loss_simple_ema"] for _, logs in tr.logged_val), "with val_ema the EMA loss is monitored"


def test_refusals(tmp_path):
    from ctrlora_amd.trainer import Trainer, validation_refusal
    kw = dict(max_steps=1, device="cpu", default_root_dir=str(tmp_path))
    with pytest.raises(ValueError, match="without val_dataloaders"):
        Trainer(val_check_interval=2, **kw).fit(_Stub(), _batches(1, 4, 1))
    with pytest.raises(ValueError, match="val_ema without an EMA"):
        Trainer(val_check_interval=2, val_ema=True, **kw).fit(_Stub(), _batches(1, 4, 1), val_dataloaders=_val_batches())
    with pytest.raises(ValueError, match="need validation"):
        Trainer(save_best=True, **kw).fit(_Stub(), _batches(1, 4, 1))
    with pytest.raises(ValueError, match="loss_bands refused"):
        Trainer(loss_bands=10, **kw).fit(_Stub(), _batches(1, 4, 1))
    for bad in (dict(val_check_interval=-1), dict(limit_val_batches=0), dict(loss_bands=65), dict(loss_bands=-1)):
        with pytest.raises(ValueError):
            Trainer(**bad, **kw)
    with pytest.raises(ValueError, match="for 500 timesteps"):
        from ctrlora_amd.validation import ValPlan
        Trainer(val_check_interval=1, val_plan=ValPlan(500), **kw).fit(_Stub(), _batches(1, 4, 1), val_dataloaders=_val_batches())

    class _Pretrain(_Stub):
        def init_data_parallel(self):
            pass

    assert validation_refusal(_Stub()) is None and "fine-tuning only" in validation_refusal(_Pretrain())
    for opts in (dict(val_check_interval=1), dict(loss_bands=4)):
        with pytest.raises(ValueError, match="fine-tuning only"):
            Trainer(**opts, **kw).fit(_Pretrain(), _batches(1, 4, 1), val_dataloaders=_val_batches())
    # validation off: val_dataloaders alone changes nothing
    tr = Trainer(**kw).fit(_Stub(), _batches(1, 4, 1), val_dataloaders=_val_batches())
    assert tr.logged_val == [] and tr.global_step == 1


def test_host_side_refusals_of_the_entry_point_need_no_gpu():
    """CL_EINVAL (1) with host addresses: every refusal of cl_loss_bands is decided before anything is launched."""
    import ctypes
    from ctrlora_amd import hip
    L = hip.lib()
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    good = dict(x=a, t=a, B=4, T=1000, nbands=10, nv=None, acc=a)
    for over in (dict(x=None), dict(t=None), dict(acc=None), dict(B=0), dict(B=65536), dict(T=0), dict(nbands=0), dict(nbands=65),
                 dict(T=5, nbands=6), dict(acc=a + 4)):
        k = dict(good, **over)
        assert L.cl_loss_bands(k["x"], k["t"], k["B"], k["T"], k["nbands"], k["nv"], k["acc"], None) == 1, over


# ------------------------------------------------------------------------------------------------ two ranks over gloo

class _Set(torch.utils.data.Dataset):
    def __init__(self, n):
        g = torch.Generator().manual_seed(5)
        self.x, self.c = torch.randn(n, 2, 2, 2, generator=g), torch.randn(n, generator=g)

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return {"x": self.x[i], "c": self.c[i]}


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _rank_worker(rank, world, port, n, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from ctrlora_amd.validation import ValPlan, reduce_tables, run_validation
        loader = torch.utils.data.DataLoader(_Set(n), batch_size=4)
        local = run_validation(_Stub(posterior=False).eval(), loader, ValPlan(T, repeats=2), rank=rank, world=world, device="cpu")
        q.put((rank, local, reduce_tables(local, world)))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_reduce_to_the_one_rank_table():
    from ctrlora_amd.validation import ValPlan, run_validation
    n, world = 23, 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, n, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in range(world)], key=lambda r: r[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    one = run_validation(_Stub(posterior=False).eval(), torch.utils.data.DataLoader(_Set(n), batch_size=4), ValPlan(T, repeats=2), device="cpu")
    (_, loc0, red0), (_, loc1, red1) = res
    assert loc0[-1, 0] == 24.0 and loc1[-1, 0] == 22.0, "samples j = r (mod 2): 12 and 11 of 23, two passes, no padding duplicates"
    assert torch.equal(red0, red1), "every rank sees the same numbers"
    assert torch.equal(red0, loc0 + loc1), "added in rank order"
    assert torch.equal(red0[:, 0], one[:, 0]) and one[-1, 0] == 46.0
    # the same 46 (x, t, noise) triples, summed in another order: the fp64 sums agree to the last few bits
    assert torch.allclose(red0, one, rtol=1e-14, atol=0.0)
