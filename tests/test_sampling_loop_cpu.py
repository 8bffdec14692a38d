"""The host logic both samplers share (ldm/models/diffusion/guided_loop.py) and what DDIMSampler / DPMSolverSampler build on
it, on CPU tensors: which apply_model calls a step makes, graphed == eager, the step hooks, the context K/V scope on every
exit, and when a captured graph is kept or released.

The kernels are replaced by plain-torch restatements of csrc/elementwise.hip (ddim_step_body, ddim_set_t_kernel,
dpmpp_step_body, dpm_set_t_kernel, tick_kernel) patched onto ctrlora_amd.hip, and guided_loop.capture by a fake whose replay()
calls the body.  A real capture calls body() once from Python without executing it; the fake calls nothing.  So here "Python-level
model calls" are the calls made outside a replay plus one body per capture, and every execution is logged with its time.
The real capture, the kernels and the S < 4 / no-engine dispatch run in tests/test_gpu_sampling_loop.py and
tests/test_gpu_dpm_solver.py."""
import contextlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from ldm.models.diffusion import guided_loop as G
from tests.dpm_solver_cases import TOL, AnalyticModel, check_case, fixture
from tests.util import rel_l2

B, SHAPE = 2, (4, 3, 5)
C, UC = torch.tensor([1.0, 0.6]), torch.tensor([-0.3, 0.2])


# ------------------------------------------------------------------------------ stand-ins

class Log:
    def __init__(self):
        self.events, self.in_replay, self.captures = [], False, 0


class FakeGraph:
    def __init__(self, body, log):
        self.body, self.log = body, log

    def replay(self):
        self.log.events.append("replay")
        self.log.in_replay = True
        try:
            self.body()
        finally:
            self.log.in_replay = False


class FakeEngine:
    """The members the samplers use: the flag, reset / detach of the cache, and the reuse key's unet.ip_layers."""
    def __init__(self, log):
        self.cache_context_kv, self.log, self.unet = False, log, SimpleNamespace(ip_layers=[])

    def reset_context_cache(self):
        self.log.events.append("reset")

    def detach_context_cache(self):
        assert self.cache_context_kv, "the kept products are taken inside the scope"
        self.log.events.append("detach")
        return "kv"


class Model:
    """eps(x, t, c) = tanh(0.7 x + 0.001 t) * c, t integer or float; c a (B,) tensor or {"c_crossattn": [tensor], ...}.
    calls: (batch size, conditioning values) of every call made outside a replay; times: t[0] of every execution.
    in_scope: every call must find the engine's context K/V flag set (cleared by tests of loops that open no scope)."""
    parameterization = "eps"

    def __init__(self, log, n=1000, fail_at=None):
        self.device, self.num_timesteps = torch.device("cpu"), n
        self.alphas_cumprod = fixture()["alphas_cumprod"].clone()[:n]
        self.alphas_cumprod_prev = torch.cat([torch.ones(1, dtype=self.alphas_cumprod.dtype), self.alphas_cumprod[:-1]])
        self.betas = torch.zeros(n)
        self.log, self.calls, self.times, self.fail_at, self.hint_scopes, self.in_scope = log, [], [], fail_at, 0, True
        eng = FakeEngine(log)
        self.engine = lambda: eng

    def apply_model(self, x, t, c):
        if self.fail_at is not None and len(self.times) == self.fail_at:
            raise RuntimeError("apply_model failed")
        assert t.shape == (x.shape[0],) and self.engine().cache_context_kv is self.in_scope
        c = c["c_crossattn"][0] if isinstance(c, dict) else c
        if not self.log.in_replay:
            self.calls.append((int(x.shape[0]), c.tolist()))
        self.times.append(float(t[0]))
        return torch.tanh(0.7 * x + 0.001 * t.float().view(-1, 1, 1, 1)) * c.view(-1, 1, 1, 1)

    @contextlib.contextmanager
    def hint_cache(self):
        self.hint_scopes += 1
        yield


def _guided(e_c, e_u, scale):
    return e_c if e_u is None else e_u + scale * (e_c - e_u)


def _ddim_row(x, e_c, e_u, noise, row, scale, x_prev, pred_x0):
    a_t, a_prev, sigma, s1m = row
    e = _guided(e_c, e_u, scale)
    p0 = (x - s1m * e) / a_t.sqrt()
    xp = a_prev.sqrt() * p0 + (1.0 - a_prev - sigma * sigma).sqrt() * e
    if noise is not None:
        xp = xp + sigma * noise
    x_prev.copy_(xp)
    if pred_x0 is not None:
        pred_x0.copy_(p0)


def _dpm_row(x, e_c, e_u, coef, i, scale, hist, x_next, pred_x0):
    alpha, sigma, cx, c0, c1, c2 = coef[i, :6]
    h = hist.view(3, -1)
    m = (x - sigma * _guided(e_c, e_u, scale)) / alpha
    xn = cx * x + c0 * m
    if float(c1) != 0.0:
        xn = xn + c1 * h[(i + 2) % 3].view_as(x)
    if float(c2) != 0.0:
        xn = xn + c2 * h[(i + 1) % 3].view_as(x)
    h[i % 3].copy_(m.reshape(-1))
    x_next.copy_(xn)
    if pred_x0 is not None:
        pred_x0.copy_(m)


@pytest.fixture
def log(monkeypatch):
    from ctrlora_amd import hip
    lg = Log()
    clamp = lambda cursor, S: min(max(int(cursor), 0), S - 1)
    ddim_index = lambda cursor, S: max(0, S - 1 - int(cursor))
    fakes = dict(
        ddim_step=lambda x, e_c, e_u, noise, coef, index, scale, x_prev, pred_x0=None:
            _ddim_row(x, e_c, e_u, noise, coef[index], scale, x_prev, pred_x0),
        ddim_step_dev=lambda x, e_c, e_u, noise, coef, cursor, S, scale, x_prev, pred_x0=None:
            _ddim_row(x, e_c, e_u, noise, coef[ddim_index(cursor, S)], scale, x_prev, pred_x0),
        ddim_set_t=lambda table, cursor, S, ts: ts.fill_(table[ddim_index(cursor, S)]),
        dpmpp_step=lambda x, e_c, e_u, coef, index, scale, hist, x_next, pred_x0=None:
            _dpm_row(x, e_c, e_u, coef, index, scale, hist, x_next, pred_x0),
        dpmpp_step_dev=lambda x, e_c, e_u, coef, cursor, S, scale, hist, x_next, pred_x0=None:
            _dpm_row(x, e_c, e_u, coef, clamp(cursor, S), scale, hist, x_next, pred_x0),
        dpm_set_t=lambda coef, cursor, S, ts: ts.fill_(coef[clamp(cursor, S), 6]),
        tick=lambda cursor: cursor.add_(1))
    for name, fn in fakes.items():
        monkeypatch.setattr(hip, name, fn)

    def capture(body):
        lg.captures += 1
        return FakeGraph(body, lg)

    monkeypatch.setattr(G, "capture", capture)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: lg.events.append("sync"))
    return lg


def _conds(kind):
    if kind == "tensor":
        return C, UC
    c, uc = {"c_crossattn": [C]}, {"c_crossattn": [UC]}
    if kind == "different":
        uc["extra"] = [UC]
    return c, uc


def _x_T():
    return torch.randn((B,) + SHAPE, generator=torch.Generator().manual_seed(3))


def _ddim(log, S, path, kind="dict", scale=7.5, sampler=None, model=None, **kw):
    """DDIMSampler.sample() on CPU tensors; path 'graphed': ddim_sampling hands its loop to _sampling_graphed as it does for
    a device tensor.  S = 3 needs a 999-step schedule (uniform spacing over 1000 steps selects 4 times for S = 3)."""
    from cldm.ddim_hacked import DDIMSampler
    model = model or Model(log, n=999 if S == 3 else 1000)
    s = sampler or DDIMSampler(model)
    if path == "graphed":
        def ddim_sampling(cond, shape, callback=None, img_callback=None, log_every_t=100, temperature=1., x_T=None,
                          unconditional_guidance_scale=1., unconditional_conditioning=None, **_):
            img = x_T.float()
            return s._sampling_graphed(cond, img, s.ddim_timesteps, callback, img_callback, log_every_t, temperature,
                                       unconditional_guidance_scale, unconditional_conditioning, {"x_inter": [img], "pred_x0": [img]})
        s.ddim_sampling = ddim_sampling
    c, uc = _conds(kind)
    out, inter = s.sample(S, B, SHAPE, c, verbose=False, eta=0.0, x_T=_x_T(), unconditional_guidance_scale=scale,
                          unconditional_conditioning=uc, **kw)
    return out, inter, model, s


def _dpm(log, S, path, kind="dict", scale=7.5, model=None):
    """DPMSolverSampler.sample() on CPU tensors, its loop for tensors outside the engine replaced by the loop under test."""
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    model = model or Model(log)
    s = DPMSolverSampler(model)
    s._loop_torch = s._loop_graphed if path == "graphed" else s._loop_eager
    c, uc = _conds(kind)
    out, _ = s.sample(S, B, SHAPE, c, verbose=False, x_T=_x_T(), unconditional_guidance_scale=scale, unconditional_conditioning=uc)
    return out, model, s


def _ddim_times(S, n):
    return [float(t) for t in reversed(range(1, n + 1, n // S))]


def _dpm_times(S):
    return [float(np.float32((t - 1e-3) * 1000.0)) for t in np.linspace(1.0, 1e-3, S + 1)[:S]]


def _expected_calls(sampler, kind, scale):
    """One step's calls by the table of DESIGN.md ("call pattern of the samplers")."""
    c, uc = C.tolist(), UC.tolist()
    if scale == 1.0:
        return [(B, c)]
    if sampler == "ddim":       # sampling: [cond; uncond], dicts only
        return [(2 * B, c + uc)] if kind == "dict" else [(B, c), (B, uc)]
    return [(B, c), (B, uc)] if kind == "different" else [(2 * B, uc + c)]      # dpm, ddim encode: [uncond; cond]


# ------------------------------------------------------------------------------ 1. the call table

# (the graphed DDIM loop keys its graph on the entries of dict conditionings: bare tensors reach the eager loop only)
@pytest.mark.parametrize("scale", [7.5, 1.0])
@pytest.mark.parametrize("S,path,kind", [(S, path, kind) for S, path in ((4, "graphed"), (4, "eager"), (3, "eager"))
                                         for kind in ("dict", "different", "tensor") if (path, kind) != ("graphed", "tensor")])
def test_ddim_sampling_calls(log, S, path, kind, scale):
    _, _, model, _ = _ddim(log, S, path, kind, scale)
    per_step = _expected_calls("ddim", kind, scale)
    python_steps = 1 if path == "graphed" else S
    assert model.calls == per_step * python_steps
    assert log.captures == (1 if path == "graphed" else 0)
    assert model.times == [t for t in _ddim_times(S, model.num_timesteps) for _ in per_step]


@pytest.mark.parametrize("scale", [7.5, 1.0])
@pytest.mark.parametrize("kind", ["dict", "different", "tensor"])
@pytest.mark.parametrize("S,path", [(4, "graphed"), (4, "eager"), (3, "eager"), (3, "torch")])
def test_dpm_calls(log, S, path, kind, scale):
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    if path == "torch":
        model = Model(log)
        model.in_scope = False          # the plain-torch loop opens no K/V scope
        c, uc = _conds(kind)
        DPMSolverSampler(model).sample(S, B, SHAPE, c, verbose=False, x_T=_x_T(), unconditional_guidance_scale=scale,
                                       unconditional_conditioning=uc)
    else:
        _, model, _ = _dpm(log, S, path, kind, scale)
    per_step = _expected_calls("dpm", kind, scale)
    assert model.calls == per_step * (1 if path == "graphed" else S)
    assert log.captures == (1 if path == "graphed" else 0)
    want = [t for t in _dpm_times(S) for _ in per_step]
    assert len(model.times) == len(want) and max(abs(a - b) for a, b in zip(model.times, want)) < 1.3e-4


@pytest.mark.parametrize("scale", [7.5, 1.0])
@pytest.mark.parametrize("kind", ["dict", "different", "tensor"])
def test_ddim_encode_calls(log, kind, scale):
    from cldm.ddim_hacked import DDIMSampler
    model = Model(log)
    model.in_scope = False              # encode opens no K/V scope
    s = DDIMSampler(model)
    s.make_schedule(4, verbose=False)
    c, uc = _conds(kind)
    s.encode(_x_T(), c, 3, unconditional_guidance_scale=scale, unconditional_conditioning=uc)
    per_step = _expected_calls("encode", kind, scale)
    assert model.calls == per_step * 3
    assert model.times == [t for t in (1.0, 251.0, 501.0) for _ in per_step]


# ------------------------------------------------------------------------------ 2. graphed == eager == a restatement

def _eps(x, t, c):
    return torch.tanh(0.7 * x + 0.001 * t) * c.view(-1, 1, 1, 1)


def _ddim_restated(S, n, scale):
    """DDIM with eta = 0 written from the method: fp64 schedule rounded to fp32 as the sampler's table is, fp32 state."""
    ac = fixture()["alphas_cumprod"].double()[:n]
    steps = list(range(1, n + 1, n // S))
    f = lambda v: torch.tensor(float(v), dtype=torch.float32)
    x = _x_T()
    for k in reversed(range(S)):
        a_t, a_prev = ac[steps[k]], (ac[steps[k - 1]] if k else ac[0])
        e_c, e_u = _eps(x, float(steps[k]), C), _eps(x, float(steps[k]), UC)
        e = e_u + scale * (e_c - e_u)
        p0 = (x - f(torch.sqrt(1 - a_t)) * e) / f(a_t).sqrt()
        x = f(a_prev).sqrt() * p0 + (1.0 - f(a_prev)).sqrt() * e
    return x


@pytest.mark.parametrize("kind", ["dict", "different"])
def test_ddim_graphed_equals_eager_and_the_restatement(log, kind):
    graphed = _ddim(log, 4, "graphed", kind)[0]
    eager = _ddim(log, 4, "eager", kind)[0]
    assert torch.equal(graphed, eager)
    for S, out in ((4, eager), (3, _ddim(log, 3, "eager", kind)[0])):
        err = rel_l2(out, _ddim_restated(S, 999 if S == 3 else 1000, 7.5))
        print(f"DDIM S={S} {kind}: rel_l2 vs the restatement {err:.3e}")
        assert err < TOL


def _dpm_case(log, name, path, steps=None):
    """Fixture case `name` (a run of the unmodified reference) through the loop under test, with the fixture's own model."""
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    case = fixture()["cases"][name]
    model = AnalyticModel("cpu", with_engine=True)
    s = DPMSolverSampler(model)
    s.order, s.skip_type = case["order"], case["skip_type"]
    s._loop_torch = {"graphed": s._loop_graphed, "eager": s._loop_eager, "torch": s._loop_torch}[path]
    x_T = case["x_T"]
    out, _ = s.sample(steps or case["S"], x_T.shape[0], tuple(x_T.shape[1:]), case["c"], verbose=False, x_T=x_T,
                      unconditional_guidance_scale=case["scale"], unconditional_conditioning=case["uc"])
    return out, model, case


def test_dpm_graphed_equals_eager_and_the_reference_run(log):
    name = "sampler_S4_cfg3.0_n420"
    graphed, model, case = _dpm_case(log, name, "graphed")
    check_case(graphed, model, case)
    eager, model_e, _ = _dpm_case(log, name, "eager")
    check_case(eager, model_e, case)
    assert torch.equal(graphed, eager)
    # S = 3 (no reference run): the eager loop over the kernels' restatement against the sampler's plain-torch loop
    err = rel_l2(_dpm_case(log, name, "eager", steps=3)[0], _dpm_case(log, name, "torch", steps=3)[0])
    print(f"DPM-Solver++ S=3: rel_l2 eager vs plain-torch loop {err:.3e}")
    assert err < TOL


# ------------------------------------------------------------------------------ 3. step hooks

def test_ddim_hooks_and_intermediates_agree_between_the_paths(log):
    runs = {}
    for path in ("graphed", "eager"):
        seen, imgs = [], []
        out, inter, _, _ = _ddim(log, 4, path, callback=seen.append, img_callback=lambda p0, i: imgs.append((i, p0.clone())),
                                 log_every_t=1)
        assert seen == [0, 1, 2, 3] and [i for i, _ in imgs] == [0, 1, 2, 3]
        assert len(inter["x_inter"]) == len(inter["pred_x0"]) == 5 and torch.equal(inter["x_inter"][-1], out)
        assert all(torch.equal(p0, kept) for (_, p0), kept in zip(imgs, inter["pred_x0"][1:]))
        runs[path] = inter
    for k in ("x_inter", "pred_x0"):
        assert len(runs["graphed"][k]) == len(runs["eager"][k])
        assert all(torch.equal(a, b) for a, b in zip(runs["graphed"][k], runs["eager"][k]))


def test_run_steps_calls_after_step_for_eager_captured_and_replayed_steps(log):
    order = []
    assert G.run_steps(lambda: order.append("body"), 4, after_step=lambda i: order.append(i)) is None
    assert order == ["body", 0, "body", 1, "body", 2, "body", 3] and log.captures == 1


# ------------------------------------------------------------------------------ 4. the context K/V scope

@pytest.mark.parametrize("fail_at", [None, 0, 2])
@pytest.mark.parametrize("sampler,path", [("ddim", "graphed"), ("ddim", "eager"), ("dpm", "graphed"), ("dpm", "eager")])
def test_context_kv_scope_is_closed_on_every_exit(log, sampler, path, fail_at):
    model = Model(log, fail_at=fail_at)
    run = (lambda: _ddim(log, 4, path, model=model)) if sampler == "ddim" else (lambda: _dpm(log, 4, path, model=model))
    if fail_at is None:
        run()
        assert len(model.times) == 4
    else:
        with pytest.raises(RuntimeError, match="apply_model failed"):
            run()
        assert len(model.times) == fail_at
    assert model.engine().cache_context_kv is False
    assert [e for e in log.events if e in ("reset", "detach")][-1] == "reset" and log.events.count("reset") == 2
    assert "detach" not in log.events


def test_context_kv_uses_two_members_and_takes_no_engine():
    eng = SimpleNamespace(cache_context_kv=False, reset_context_cache=lambda: None)
    with G.context_kv(eng) as e:
        assert e is eng and eng.cache_context_kv is True
    assert eng.cache_context_kv is False
    with G.context_kv(G.engine_of(SimpleNamespace())) as e:
        assert e is None


def test_hint_scope_is_entered_once_per_call_when_hoisting(log):
    for hoist, want in ((True, 1), (False, 0)):
        from cldm.ddim_hacked import DDIMSampler
        model = Model(log)
        s = DDIMSampler(model)
        s.hoist_hint_encode = hoist
        _ddim(log, 4, "eager", sampler=s, model=model)
        assert model.hint_scopes == want
    with G.hint_scope(SimpleNamespace(), True):         # a model that offers no hint cache
        pass


# ------------------------------------------------------------------------------ 5. keeping and releasing the graph

@pytest.mark.parametrize("sampler", ["ddim", "dpm"])
def test_a_graph_that_is_not_kept_is_released_after_a_synchronize(log, sampler):
    s = (_ddim(log, 4, "graphed")[3] if sampler == "ddim" else _dpm(log, 4, "graphed")[2])
    assert log.events.count("replay") == 3 and log.events.count("sync") == 1
    tail = [e for e in log.events if e != "reset"]
    assert tail[-2:] == ["replay", "sync"]              # nothing replays after the wait; the K/V scope closes after it
    assert log.events[-1] == "reset"
    assert getattr(s, "_graph_state", None) is None


def test_ddim_reuse_graph_keeps_the_graph_and_the_second_call_only_replays(log):
    from cldm.ddim_hacked import DDIMSampler
    model = Model(log)
    s = DDIMSampler(model)
    s.reuse_graph = True
    first = _ddim(log, 4, "graphed", sampler=s, model=model)[0]
    assert "sync" not in log.events and isinstance(s._graph_state["graph"], FakeGraph) and s._graph_state["kv"] == "kv"
    kv = [e for e in log.events if e in ("reset", "detach")]
    assert kv == ["reset", "detach", "reset"] and model.engine().cache_context_kv is False
    assert len(model.calls) == 1 and log.captures == 1 and s.graph_hits == 0
    del log.events[:]
    model.in_scope = False              # a hit opens no K/V scope: the kept graph reads the products it holds
    second = _ddim(log, 4, "graphed", sampler=s, model=model)[0]
    assert log.events == ["replay"] * 4                 # S replays: no capture, no wait, no K/V scope
    assert len(model.calls) == 1 and log.captures == 1 and s.graph_hits == 1 and len(model.times) == 8
    assert torch.equal(second, first)
    assert torch.equal(first, _ddim(log, 4, "eager")[0])
