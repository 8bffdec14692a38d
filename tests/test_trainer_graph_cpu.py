"""`Trainer(graph_step=...)` without a GPU: the script flag, the refusals that need no device, the untouched default loop, and the
micro-step bookkeeping of the graphed loop driven with a recording stand-in for the captured step (which micro-step clears the
gradients, which one exchanges and optimizes, when the graphs are captured, when `global_step` advances, what the counters
count, how often the callbacks fire).  tests/test_gpu_trainer_graph.py runs the real thing."""
import importlib.util
import os

import pytest
import torch
import torch.nn as nn

from tests.util import ROOT


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


NEED = ["--dataroot", "d", "--config", "c", "--sd_ckpt", "s", "--cn_ckpt", "n"]


def test_parser_accepts_graph_and_defaults_to_off():
    p = _script("train_ctrlora_finetune").get_parser()
    assert p.parse_args(NEED).graph is False
    assert p.parse_args(NEED + ["--graph"]).graph is True
    assert p.parse_args(NEED + ["--graph", "--gradacc", "4", "--latent_cache", "x"]).gradacc == 4
    help_text = " ".join(p.format_help().split())
    assert "--graph" in help_text and "hipGraph" in help_text and "replay" in help_text


def test_cpu_device_is_refused_with_the_reason():
    from ctrlora_amd.trainer import Trainer
    for arg in (True, dict(warm_steps=1)):
        with pytest.raises(ValueError, match="needs a GPU.*cpu"):
            Trainer(graph_step=arg, device="cpu")
    with pytest.raises(ValueError, match="unknown option.*warmup"):
        Trainer(graph_step=dict(warmup=1), device="cpu")
    tr = Trainer(device="cpu")
    assert tr.graph_step is False and tr.graph_mode == "off" and tr.graph_replays == 0 and tr.graph_eager_steps == 0


def test_refusal_reasons_name_what_is_wrong():
    from ctrlora_amd.trainer import graph_step_refusal

    class Fine:
        loss_type, original_elbo_weight = "l2", 0.0

        def engine_train_step(self, *a):
            pass

    class L1(Fine):
        loss_type = "l1"

    class Elbo(Fine):
        original_elbo_weight = 0.5

    class Pretrain(Fine):
        def init_data_parallel(self):
            pass

    assert graph_step_refusal(Fine()) is None
    assert "loss_type is 'l1'" in graph_step_refusal(L1())
    assert "original_elbo_weight is 0.5" in graph_step_refusal(Elbo())
    assert "pre-training" in graph_step_refusal(Pretrain())
    assert "no engine_train_step" in graph_step_refusal(object())
    assert all("\n" not in graph_step_refusal(m) for m in (L1(), Elbo(), Pretrain(), object()))


class _Toy(nn.Module):
    """LightningModule-shaped toy for the default loop: loss = mean((x.w - y)^2)."""

    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(3))
        self.args = []

    def training_step(self, batch, batch_idx):
        self.args.append((batch, batch_idx))
        return ((batch["x"] @ self.w - batch["y"]) ** 2).mean()

    def configure_optimizers(self):
        return torch.optim.SGD(self.parameters(), lr=0.1)


def _toy_batches(n):
    g = torch.Generator().manual_seed(0)
    return [dict(x=torch.randn(2, 3, generator=g), y=torch.randn(2, generator=g)) for _ in range(n)]


def test_default_trainer_runs_the_existing_loop_and_never_builds_a_step_object(tmp_path, monkeypatch):
    from ctrlora_amd import trainer as T
    monkeypatch.setattr(T.Trainer, "_fit_graphed", lambda *a, **k: pytest.fail("the graphed loop ran without graph_step"))
    monkeypatch.setattr(T.Trainer, "_make_graph_step", lambda *a, **k: pytest.fail("a step object was built without graph_step"))
    batches = _toy_batches(2)
    model = _Toy()
    tr = T.Trainer(max_steps=2, default_root_dir=str(tmp_path), device="cpu", log_every_n_steps=1)
    tr.fit(model, batches)
    assert tr.global_step == 2 and [i for _, i in model.args] == [0, 1]
    # training_step got the loader's own batches and an index: nothing else, no graph object
    assert all(b is want for (b, _), want in zip(model.args, batches))
    assert float(model.w.detach().abs().sum()) > 0 and len(tr.logged) == 2
    assert tr.graph_mode == "off" and tr.graph_replays == 0 and tr.graph_eager_steps == 0
    assert not hasattr(tr, "_graph_step_obj")


class _FakeStep:
    """Stands where GraphedTrainStep stands in Trainer._fit_graphed and records what it is asked to do."""
    mode = "one"

    def __init__(self, tensors):
        self.shapes = [t.shape for t in tensors]
        self.captured = False
        self.calls = []

    def matches(self, *tensors):
        return [t.shape for t in tensors] == self.shapes

    def capture(self):
        assert not self.captured
        self.captured = True
        self.calls.append(("capture",))

    def _run(self, kind, z, first, last):
        self.calls.append((kind, int(z[0, 0]), first, last))
        return torch.tensor([0.5, 0.25, float(z[0, 0])])

    def eager(self, z, ctx, hint, t, noise, first=True, last=True):
        return self._run("eager", z, first, last)

    def micro(self, z, ctx, hint, t, noise, first=True, last=True):
        assert self.captured
        return self._run("replay", z, first, last)


class _GraphToy(nn.Module):
    """What the graphed loop touches of a model: get_input, _hint_latent, num_timesteps, log_dict, device."""
    first_stage_key, num_timesteps, device = "jpg", 1000, torch.device("cpu")

    def __init__(self):
        super().__init__()
        self.logged = []

    def get_input(self, batch, k):
        return batch[k], {"c_crossattn": [batch["ctx"]], "c_concat": [batch["hint"]]}

    def _hint_latent(self, cond):
        return cond["c_concat"][0]

    def log_dict(self, d):
        self.logged.append({k: float(v) for k, v in d.items()})


class _Events:
    def __init__(self):
        self.batch_end, self.steps_at_batch_end, self.n_batch_end = [], [], 0

    def on_train_batch_end(self, trainer, module, outputs, batch, batch_idx):
        self.batch_end.append(float(outputs["loss"]))
        self.steps_at_batch_end.append(trainer.global_step)

    def on_batch_end(self, trainer, module):
        self.n_batch_end += 1


def _graph_batches(n, odd=()):
    # batch i carries the value i in z[0, 0]; the batches in `odd` have another batch size
    return [dict(jpg=torch.full((3 if i in odd else 2, 4), float(i)), ctx=torch.zeros(3 if i in odd else 2, 5),
                 hint=torch.zeros(3 if i in odd else 2, 4)) for i in range(n)]


def _drive(acc, steps, warm=2, odd=(), tmp="."):
    from ctrlora_amd.trainer import Trainer
    ev = _Events()
    tr = Trainer(max_steps=steps, accumulate_grad_batches=acc, default_root_dir=tmp, device="cpu", log_every_n_steps=1, callbacks=[ev])
    tr._graph_opts = dict(warm_steps=warm)
    made = []
    tr._make_graph_step = lambda model, tensors: (made.append(_FakeStep(tensors)), made[-1])[1]
    model = _GraphToy()
    tr._fit_graphed(model, _graph_batches(acc * steps, odd))
    assert len(made) == 1, "one step object per fit"
    return tr, made[0], model, ev


@pytest.mark.parametrize("acc", [1, 2, 3])
def test_micro_step_bookkeeping(acc, tmp_path):
    steps = 5
    tr, fake, model, ev = _drive(acc, steps, tmp=str(tmp_path))
    runs = [c for c in fake.calls if c[0] != "capture"]
    # every batch exactly once, in order: none spent on warm-up, none consumed twice
    assert [c[1] for c in runs] == list(range(acc * steps))
    # the first micro-step of an optimizer step clears, the last one exchanges + optimizes, the ones between do neither
    assert [c[2] for c in runs] == [i % acc == 0 for i in range(acc * steps)]
    assert [c[3] for c in runs] == [i % acc == acc - 1 for i in range(acc * steps)]
    # two optimizer steps launched eagerly, each on its own batches; captured once, at a step boundary; replays from there on
    assert [c[0] for c in runs] == ["eager"] * (2 * acc) + ["replay"] * ((steps - 2) * acc)
    assert fake.calls.index(("capture",)) == 2 * acc and fake.calls.count(("capture",)) == 1
    assert tr.global_step == steps and tr.graph_eager_steps == 2 and tr.graph_replays == steps - 2 and tr.graph_mode == "one"
    # global_step advances after the last micro-step only; callbacks fire once per micro-batch and see the device scalar
    assert ev.steps_at_batch_end == [(i + 1) // acc for i in range(acc * steps)]
    assert ev.n_batch_end == acc * steps and ev.batch_end == [float(i) for i in range(acc * steps)]
    assert [d["train/loss"] for d in model.logged] == [float(i) for i in range(acc * steps)]
    assert set(model.logged[0]) == {"train/loss_simple", "train/loss_vlb", "train/loss"}
    assert [s for s, _ in tr.logged] == list(range(1, steps + 1))
    assert [v for _, v in tr.logged] == [float(acc * (s + 1) - 1) for s in range(steps)]


def test_a_batch_of_another_shape_is_launched_eagerly_and_counted(tmp_path):
    # acc 2, batch 7 (second micro-step of optimizer step 4) has another batch size: that step counts as eager, the next replays
    tr, fake, _, _ = _drive(2, 6, odd=(7,), tmp=str(tmp_path))
    runs = [c for c in fake.calls if c[0] != "capture"]
    assert [c[0] for c in runs] == ["eager"] * 4 + ["replay"] * 3 + ["eager"] + ["replay"] * 4
    assert runs[7] == ("eager", 7, False, True)
    assert tr.graph_eager_steps == 3 and tr.graph_replays == 3 and tr.global_step == 6


def test_capture_waits_for_a_batch_of_the_first_batch_s_shape(tmp_path):
    # warm_steps 1: the capture is due at batch 1, which has another shape -> that step is eager, the capture follows at batch 2
    tr, fake, _, _ = _drive(1, 4, warm=1, odd=(1,), tmp=str(tmp_path))
    assert [c[0] for c in fake.calls] == ["eager", "eager", "capture", "replay", "replay"]
    assert tr.graph_eager_steps == 2 and tr.graph_replays == 2


def test_warm_steps_zero_captures_before_the_first_step(tmp_path):
    tr, fake, _, _ = _drive(2, 2, warm=0, tmp=str(tmp_path))
    assert [c[0] for c in fake.calls] == ["capture"] + ["replay"] * 4
    assert tr.graph_eager_steps == 0 and tr.graph_replays == 2
