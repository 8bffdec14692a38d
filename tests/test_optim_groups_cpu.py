"""Parameter groups and the device learning-rate schedule of FusedAdamW, without a GPU: the group rules on the real name lists, the
chunk -> group map, what the optimizer launches (a recorder in place of the library), sync_hyper, the state dict, and the host-side
refusals of the two new entry points against the built library."""
import ctypes
import json
import os
from types import SimpleNamespace

import pytest
import torch

from tests.util import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")
LORA_PLUS = {"name": "lora_up", "match": ["lora_layer.up."], "lr_scale": 4.0}
NO_DECAY = {"name": "no_decay", "match": ["norm", ".bias"], "weight_decay": 0.0}


def _names(which, **flags):
    """trainable_names() of ControlFinetuneLDM over the recorded ControlNet key list (name -> shape)."""
    from cldm.cldm_ctrlora_finetune import ControlFinetuneLDM
    keys = json.load(open(os.path.join(GOLDEN, which)))["controlnet"]
    cm = SimpleNamespace(named_parameters=lambda: [(k, None) for k in keys], ft_with_lora=True,
                         norm_trainable=flags.get("norm", True), zero_trainable=flags.get("zero", True))
    return ControlFinetuneLDM.trainable_names(SimpleNamespace(control_model=cm)), keys


def _trainable_set(names, shapes, device):
    from ctrlora_amd.engine.packing import TrainableSet
    ts = TrainableSet()
    for n in names:
        ts.declare(n, shapes[n])
    ts.materialize({n: torch.zeros(shapes[n], device=device) for n in names}, device)
    return ts


# ------------------------------------------------------------------------------------------------ group rules

@pytest.mark.parametrize("which", ["keys_tiny.json", "keys_sd15.json"])
def test_rules_partition_the_real_trainable_set(which):
    from cldm.cldm_ctrlora_finetune import assign_optim_groups
    names, keys = _names(which)
    assert len(names) == 164 + 56 + 26, "82 LoRA pairs, the norm layers, the zero convs"
    groups = assign_optim_groups(names, [LORA_PLUS, NO_DECAY])
    assert [g["name"] for g in groups] == ["default", "lora_up", "no_decay"]
    assert [(g["lr_scale"], g["weight_decay"]) for g in groups] == [(1.0, None), (4.0, None), (1.0, 0.0)]
    members = [n for g in groups for n in g["names"]]
    assert sorted(members) == sorted(names) and len(set(members)) == len(names), "every name in exactly one group"
    assert groups[1]["names"] == [n for n in names if n.endswith("lora_layer.up.weight")] and len(groups[1]["names"]) == 82
    assert groups[2]["names"] == [n for n in names if "lora_layer.up." not in n and ("norm" in n or ".bias" in n)]
    assert all("lora_layer.down" in n or (("zero_convs" in n or "middle_block_out" in n) and n.endswith(".weight")) for n in groups[0]["names"])
    # order inside a group is trainable_names()' order, and the first match wins
    first = assign_optim_groups(names, [dict(NO_DECAY, match=["lora_layer", "norm"]), LORA_PLUS | {"match": ["zero_convs"]}])
    assert not any("lora_layer" in n for n in first[2]["names"]) and all("zero_convs" in n for n in first[2]["names"])
    # no rules: one group, everything
    (only,) = assign_optim_groups(names, [])
    assert only["names"] == names and only["name"] == "default"
    # frozen norms: the no-decay rule still finds the zero convs' biases
    frozen, _ = _names(which, norm=False)
    assert len(assign_optim_groups(frozen, [NO_DECAY])[1]["names"]) == 13


def test_rules_that_cannot_be_meant_are_refused():
    from cldm.cldm_ctrlora_finetune import assign_optim_groups
    names, _ = _names("keys_tiny.json")
    with pytest.raises(ValueError, match="'typo'.*takes none"):
        assign_optim_groups(names, [{"name": "typo", "match": ["lora_layer.upp."]}])
    with pytest.raises(ValueError, match="'second'.*takes none"):
        assign_optim_groups(names, [LORA_PLUS, dict(LORA_PLUS, name="second")])
    with pytest.raises(ValueError, match="must differ"):
        assign_optim_groups(names, [LORA_PLUS, dict(NO_DECAY, name="lora_up")])
    with pytest.raises(ValueError, match="must differ"):
        assign_optim_groups(names, [dict(LORA_PLUS, name="default")])
    with pytest.raises(ValueError, match="at most 8"):
        assign_optim_groups(names, [{"name": f"g{i}", "match": [f"zero_convs.{i}."]} for i in range(8)])
    assert len(assign_optim_groups(names, [{"name": f"g{i}", "match": [f"zero_convs.{i}."]} for i in range(7)])) == 8
    for bad in ({"match": ["x"]}, {"name": "a"}, {"name": "a", "match": []}, {"name": "a", "match": ["x"], "lr": 1.0},
                dict(LORA_PLUS, lr_scale=0.0), dict(LORA_PLUS, lr_scale=-1.0), dict(NO_DECAY, weight_decay=-0.1)):
        with pytest.raises(ValueError):
            assign_optim_groups(names, [bad])


def test_pretraining_refuses_both_options_and_finetuning_keeps_them():
    import bench
    for opt in (dict(optim_groups=[LORA_PLUS]), dict(scheduler_config={"target": "ctrlora_amd.lr_schedule.WarmupDecay",
                                                                       "params": dict(kind="linear", warmup_steps=0, total_steps=4)})):
        with pytest.raises(NotImplementedError, match="fine-tuning only.*ControlPretrainLDM"):
            bench.build_model("ctrlora_pretrain_sd15_9tasks_rank128.yaml", 0, tiny=True, mutate=lambda p: p.update(opt))
    m = bench.build_model("ctrlora_finetune_sd15_rank128.yaml", 0, tiny=True, mutate=lambda p: p.update(optim_groups=[LORA_PLUS, NO_DECAY]))
    assert m.optim_groups == [LORA_PLUS, NO_DECAY] and m.scheduler_config is None
    plain = bench.build_model("ctrlora_finetune_sd15_rank128.yaml", 0, tiny=True)
    assert plain.optim_groups is None and plain.scheduler_config is None and plain.use_scheduler is False
    # the names of the built model are the recorded list's: the rules see what the golden test saw
    assert sorted(m.trainable_names()) == sorted(_names("keys_tiny.json")[0])


# ------------------------------------------------------------------------------------------------ the chunk -> group map

@pytest.mark.parametrize("which,device", [("keys_tiny.json", "cpu"), ("keys_sd15.json", "meta")])
def test_chunk_group_map_follows_every_trainable(which, device):
    from cldm.cldm_ctrlora_finetune import assign_optim_groups
    from ctrlora_amd.engine.packing import rup
    from ctrlora_amd.train import build_chunk_group
    names, shapes = _names(which)
    groups = assign_optim_groups(names, [LORA_PLUS, NO_DECAY])
    group_of = {n: k for k, g in enumerate(groups) for n in g["names"]}
    ts = _trainable_set(list(reversed(names)), shapes, device)            # any layout order: the map follows the offsets
    cg = build_chunk_group(ts.items, ts.numel, group_of, 3)
    assert cg.dtype == torch.uint8 and cg.numel() * 64 == ts.numel and ts.numel % 64 == 0
    covered = 0
    for t in ts.items:
        n = int(torch.Size(t.shape).numel())
        lo, hi = t.offset // 64, (t.offset + rup(n, 64)) // 64
        assert t.offset % 64 == 0 and bool((cg[lo:hi] == group_of[t.name]).all()), t.name
        covered += hi - lo
    assert covered == cg.numel(), "the tensors and their padding tile the buffer: no chunk is left to a default"
    assert sorted(set(cg.tolist())) == [0, 1, 2]
    if which == "keys_sd15.json":
        assert ts.numel == sum(rup(int(torch.Size(shapes[n]).numel()), 64) for n in names) and 36.9e6 < ts.numel < 37.0e6
    # the host builder refuses what the kernel would have to clamp, and what it cannot place
    with pytest.raises(ValueError, match="names group 3, the table has 3"):
        build_chunk_group(ts.items, ts.numel, {**group_of, names[0]: 3}, 3)
    with pytest.raises(ValueError, match="in no parameter group"):
        build_chunk_group(ts.items, ts.numel, {n: k for n, k in group_of.items() if n != names[5]}, 3)
    with pytest.raises(ValueError, match="1 to 8"):
        build_chunk_group(ts.items, ts.numel, group_of, 9)
    with pytest.raises(ValueError, match="whole number"):
        build_chunk_group(ts.items, ts.numel + 8, group_of, 3)
    moved = SimpleNamespace(name=names[0], shape=ts.items[0].shape, offset=ts.items[0].offset + 32)
    with pytest.raises(ValueError, match="whole chunks"):
        build_chunk_group([moved], ts.numel, group_of, 3)


# ------------------------------------------------------------------------------------------------ what FusedAdamW launches

SHAPES = {"a.lora_layer.down.weight": (8, 20), "a.lora_layer.up.weight": (20, 8), "n.norm.weight": (70,), "n.norm.bias": (70,),
          "zero_convs.0.0.weight": (4, 4, 1, 1), "b.lora_layer.up.weight": (3, 8)}


def _bound_ex(seed=0):
    """A bank on the host laid out by the real TrainableSet, with nn.Parameters bound to it the way bind_trainables binds them."""
    ts = _trainable_set(list(SHAPES), SHAPES, "cpu")
    g = torch.Generator().manual_seed(seed)
    ts.flat.copy_(torch.randn(ts.numel, generator=g))
    ts.flat_grad.copy_(torch.randn(ts.numel, generator=g))
    params = {}
    for t in ts.items:
        p = torch.nn.Parameter(torch.zeros(0))
        p.data, p.grad = t.master, t.grad
        params[t.name] = p
    return SimpleNamespace(tr=ts, repack=lambda: None), params


def _grouped(params, lr=1e-3):
    up = [p for n, p in params.items() if "lora_layer.up." in n]
    nd = [p for n, p in params.items() if "norm" in n]
    rest = [p for n, p in params.items() if "lora_layer.up." not in n and "norm" not in n]
    return [dict(params=rest, name="default"), dict(params=up, name="lora_up", lr=4 * lr), dict(params=nd, name="no_decay", weight_decay=0.0)]


@pytest.fixture
def rec(monkeypatch):
    from ctrlora_amd import hip
    from tests.test_engine_launch_sequence import Recorder
    r = Recorder({})
    monkeypatch.setattr(hip, "_lib", r)
    monkeypatch.setattr(hip, "stream", lambda: 0)
    return r


def test_one_group_and_no_schedule_launch_what_they_did(rec):
    from ctrlora_amd.train import FusedAdamW
    ex, params = _bound_ex()
    for form in (list(params.values()), [dict(params=list(params.values()))]):
        opt = FusedAdamW(form, [ex], lr=1e-3)
        assert opt._chunk_group is None and opt._lr_table is None and opt.group_names == ["default"]
        assert tuple(opt._hyper_table.shape) == (1, 6) and opt._hyper.data_ptr() == opt._hyper_table.data_ptr() and tuple(opt._hyper.shape) == (6,)
        assert "name" not in opt.state_dict()["param_groups"][0], "one group: the state dict of before"
        rec.clear()
        opt.step()
        assert [(n, len(a)) for n, a in rec.calls] == [("cl_tick", 2), ("cl_adamw_dev", 8)]
        st = opt._states[0]
        assert rec.calls[1][1][:7] == (ex.tr.flat.data_ptr(), ex.tr.flat_grad.data_ptr(), st.m.data_ptr(), st.v.data_ptr(), ex.tr.numel,
                                       opt._hyper.data_ptr(), opt._step_dev.data_ptr())
        opt.max_grad_norm = 1.0
        rec.clear()
        opt.step()
        assert [n for n in rec.names() if n != "cl_grad_norm_scratch_floats"] == ["cl_grad_norm", "cl_tick", "cl_adamw_dev_clip"]
        assert opt.last_lr().data_ptr() == opt._hyper.data_ptr() and opt.last_lr().tolist() == [float(torch.tensor(1e-3))]


def test_groups_launch_the_grouped_kernel_with_table_and_map(rec):
    from ctrlora_amd.train import FusedAdamW
    from ldm.modules.ema import ModelEma
    ex, params = _bound_ex()
    opt = FusedAdamW(_grouped(params), [ex], lr=1e-3, weight_decay=1e-2, grad_scale=0.5)
    assert opt.group_names == ["default", "lora_up", "no_decay"] and tuple(opt._hyper_table.shape) == (3, 6)
    f = lambda x: float(torch.tensor(x, dtype=torch.float32))
    assert opt._hyper_table.tolist() == [[f(1e-3), f(0.9), f(0.999), f(1e-8), f(1e-2), 0.5], [f(4e-3), f(0.9), f(0.999), f(1e-8), f(1e-2), 0.5],
                                         [f(1e-3), f(0.9), f(0.999), f(1e-8), 0.0, 0.5]]
    assert opt._hyper.data_ptr() == opt._hyper_table.data_ptr() and opt._hyper.tolist() == opt._hyper_table[0].tolist()
    (cg,) = opt._chunk_group
    want = {"a.lora_layer.down.weight": 0, "a.lora_layer.up.weight": 1, "n.norm.weight": 2, "n.norm.bias": 2, "zero_convs.0.0.weight": 0,
            "b.lora_layer.up.weight": 1}
    for t in ex.tr.items:
        assert set(cg[t.offset // 64:(t.offset + t.master.numel() + 63) // 64].tolist()) == {want[t.name]}, t.name
    opt.step()
    assert rec.names() == ["cl_tick", "cl_adamw_dev_groups"]
    st = opt._states[0]
    (a,) = rec.of("cl_adamw_dev_groups")
    assert a[:10] == (ex.tr.flat.data_ptr(), ex.tr.flat_grad.data_ptr(), st.m.data_ptr(), st.v.data_ptr(), ex.tr.numel,
                      opt._hyper_table.data_ptr(), 3, cg.data_ptr(), opt._step_dev.data_ptr(), None), "no clipping: clip is NULL"
    # clipping passes grad_norm_out; the norm still reads row 0 (grad_scale is common to all groups)
    opt.max_grad_norm = 1.0
    rec.clear()
    opt.step()
    assert [n for n in rec.names() if n != "cl_grad_norm_scratch_floats"] == ["cl_grad_norm", "cl_tick", "cl_adamw_dev_groups"]
    assert rec.of("cl_grad_norm")[0][3] == opt._hyper.data_ptr()
    assert rec.of("cl_adamw_dev_groups")[0][9] == opt.grad_norm_out.data_ptr()
    # a schedule inserts cl_lr_schedule after the tick and before the first AdamW launch; the EMA launches follow as before
    ema = ModelEma([("a", ex.tr.flat)], decay=0.9)
    shadow = torch.zeros_like(ex.tr.flat)
    opt.attach_ema(ema, [shadow])
    opt.set_lr_schedule(torch.full((5, 3), 1e-4))
    rec.clear()
    opt.step()
    names = [n for n in rec.names() if n != "cl_grad_norm_scratch_floats"]
    assert names == ["cl_grad_norm", "cl_tick", "cl_lr_schedule", "cl_tick", "cl_adamw_dev_groups", "cl_ema_update"], names
    (s,) = rec.of("cl_lr_schedule")
    assert s[:5] == (opt._hyper_table.data_ptr(), 3, opt._lr_table.data_ptr(), 5, opt._step_dev.data_ptr())
    assert [t[0] for t in rec.of("cl_tick")] == [opt._step_dev.data_ptr(), ema.num_updates.data_ptr()]
    assert rec.of("cl_ema_update")[0][:3] == (shadow.data_ptr(), ex.tr.flat.data_ptr(), ex.tr.numel)


def test_a_schedule_on_one_group_keeps_the_one_group_kernel(rec):
    from ctrlora_amd.train import FusedAdamW
    ex, params = _bound_ex()
    opt = FusedAdamW(list(params.values()), [ex], lr=1e-3)
    opt.set_lr_schedule([1e-4, 2e-4, 3e-4])           # [T]: broadcast over the groups
    assert tuple(opt._lr_table.shape) == (3, 1)
    opt.step()
    assert rec.names() == ["cl_tick", "cl_lr_schedule", "cl_adamw_dev"]
    assert rec.of("cl_adamw_dev")[0][5] == opt._hyper.data_ptr() == rec.of("cl_lr_schedule")[0][0]
    opt.set_lr_schedule(None)
    rec.clear()
    opt.step()
    assert rec.names() == ["cl_tick", "cl_adamw_dev"]


def test_membership_is_checked_like_torch():
    from ctrlora_amd.train import FusedAdamW
    ex, params = _bound_ex()
    groups = _grouped(params)
    with pytest.raises(ValueError, match="more than one parameter group"):
        FusedAdamW([groups[0], dict(groups[1], params=groups[1]["params"] + groups[0]["params"][:1]), groups[2]], [ex])
    with pytest.raises(ValueError, match="2 trainable tensors are in no parameter group.*n.norm"):
        FusedAdamW(groups[:2], [ex])
    with pytest.raises(ValueError, match="at most 8"):
        FusedAdamW([dict(params=[torch.nn.Parameter(torch.zeros(1))]) for _ in range(9)], [ex])
    with pytest.raises(ValueError, match="distinct names"):
        FusedAdamW([groups[0], dict(groups[1], name="default"), groups[2]], [ex])


# ------------------------------------------------------------------------------------------------ sync_hyper, the schedule's rules

def test_sync_hyper_pushes_any_group_and_leaves_a_scheduled_lr_alone(rec):
    from ctrlora_amd.train import FusedAdamW
    ex, params = _bound_ex()
    opt = FusedAdamW(_grouped(params), [ex], lr=1e-3)
    f = lambda x: float(torch.tensor(x, dtype=torch.float32))
    before = opt._hyper_table.clone()
    opt.param_groups[2]["lr"] = 7e-4
    opt.param_groups[1]["betas"] = (0.8, 0.95)
    assert torch.equal(opt._hyper_table, before), "nothing moves until sync_hyper()"
    opt.step()                                           # outside a capture the step syncs
    assert opt._hyper_table[2, 0].item() == f(7e-4) and opt._hyper_table[1, 1:3].tolist() == [f(0.8), f(0.95)]
    assert torch.equal(opt._hyper_table[0], before[0]) and opt._hyper_table[1, 0] == before[1, 0]
    assert opt.last_lr().tolist() == [f(1e-3), f(4e-3), f(7e-4)] and opt.last_lr().data_ptr() == opt._hyper_table.data_ptr()
    # with a table set the device owns the lr column: the host mirror does not reach it, the other columns still do
    table = torch.tensor([[1e-4, 2e-4, 3e-4], [4e-4, 5e-4, 6e-4]])
    opt.set_lr_schedule(table)
    assert opt._lr_table is not table and torch.equal(opt._lr_table, table)
    opt._hyper_table[:, 0] = torch.tensor([9.0, 8.0, 7.0])        # what cl_lr_schedule would have written
    for g in opt.param_groups:
        g["lr"] = 0.5
    opt.param_groups[0]["weight_decay"] = 0.25
    opt.sync_hyper()
    assert opt._hyper_table[:, 0].tolist() == [9.0, 8.0, 7.0] and opt._hyper_table[0, 4].item() == 0.25
    # new values of the same shape go into the same tensor; another shape is a new tensor (before any capture)
    ptr = opt._lr_table.data_ptr()
    opt.set_lr_schedule(table * 2)
    assert opt._lr_table.data_ptr() == ptr and torch.equal(opt._lr_table, table * 2)
    opt.set_lr_schedule(torch.ones(4, 3))
    assert tuple(opt._lr_table.shape) == (4, 3)
    for bad in (torch.ones(4, 2), torch.ones(0, 3), torch.ones(2, 3, 1)):
        with pytest.raises(ValueError, match=r"\[T\] or \[T, 3\]"):
            opt.set_lr_schedule(bad)
    # dropping the schedule hands the column back to the host mirror
    opt.set_lr_schedule(None)
    assert opt._hyper_table[:, 0].tolist() == [0.5, 0.5, 0.5]
    # after a capture only the values may change
    opt.set_lr_schedule(torch.ones(4, 3))
    opt._captured = True
    opt.set_lr_schedule(torch.zeros(4, 3))
    assert float(opt._lr_table.sum()) == 0.0
    with pytest.raises(RuntimeError, match="after a capture.*same shape"):
        opt.set_lr_schedule(torch.ones(5, 3))
    with pytest.raises(RuntimeError, match="after a capture.*launches cl_lr_schedule"):
        opt.set_lr_schedule(None)
    ex2, params2 = _bound_ex()
    opt2 = FusedAdamW(_grouped(params2), [ex2], lr=1e-3)
    opt2._captured = True
    with pytest.raises(RuntimeError, match="after a capture.*does not launch cl_lr_schedule"):
        opt2.set_lr_schedule(torch.ones(4, 3))
    opt2.set_lr_schedule(None)        # nothing set, nothing to drop


# ------------------------------------------------------------------------------------------------ state

def test_state_round_trip_with_groups_and_refusal_of_another_structure(rec):
    from ctrlora_amd.train import FusedAdamW, PretrainAdamW
    ex, params = _bound_ex()
    opt = FusedAdamW(_grouped(params), [ex], lr=1e-3)
    opt._states[0].m.copy_(torch.arange(ex.tr.numel, dtype=torch.float32))
    opt._states[0].v.fill_(2.0)
    opt._step_dev.fill_(5)
    opt.param_groups[1]["lr"] = 3e-3
    sd = opt.state_dict()
    assert [g["name"] for g in sd["param_groups"]] == ["default", "lora_up", "no_decay"]
    assert [g["lr"] for g in sd["param_groups"]] == [1e-3, 3e-3, 1e-3] and sd["param_groups"][2]["weight_decay"] == 0.0
    assert all("params" not in g for g in sd["param_groups"])
    ex2, params2 = _bound_ex(1)
    new = FusedAdamW(_grouped(params2, lr=5e-4), [ex2], lr=5e-4)
    new.load_state_dict(sd)
    a, b = new._states[0].export(), opt._states[0].export()       # by name: the padding between the tensors is not state
    assert int(new._step_dev) == 5 and all(torch.equal(a[k][n], b[k][n]) for k in ("m", "v") for n in SHAPES)
    opt.sync_hyper()
    assert [g["lr"] for g in new.param_groups] == [1e-3, 3e-3, 1e-3] and torch.equal(new._hyper_table, opt._hyper_table)
    # another group structure: refused before the first copy, naming the difference
    one = FusedAdamW(list(_bound_ex(2)[1].values()), [ex2], lr=5e-4)
    keep = (one._states[0].m.clone(), int(one._step_dev), one._hyper_table.clone())
    with pytest.raises(ValueError, match=r"\['default', 'lora_up', 'no_decay'\].*\['default'\]"):
        one.load_state_dict(sd)
    assert torch.equal(one._states[0].m, keep[0]) and int(one._step_dev) == keep[1] and torch.equal(one._hyper_table, keep[2])
    with pytest.raises(ValueError, match=r"\['default'\].*\['default', 'lora_up', 'no_decay'\]"):
        new.load_state_dict(one.state_dict())
    assert int(new._step_dev) == 5
    # a one-group state of before (no names, or no param_groups at all) still loads into a one-group optimizer
    old = one.state_dict()
    assert "name" not in old["param_groups"][0]
    one.load_state_dict(old)
    one.load_state_dict({k: v for k, v in old.items() if k != "param_groups"})
    # pre-training: one group, no device schedule
    base = SimpleNamespace(tr=ex.tr, repack=lambda: None)
    with pytest.raises(NotImplementedError, match="fine-tuning only"):
        PretrainAdamW(_grouped(params), base, {})
    pre = PretrainAdamW(list(params.values()), base, {})
    with pytest.raises(NotImplementedError, match="fine-tuning only"):
        pre.set_lr_schedule(torch.ones(3))
    pre.set_lr_schedule(None)


# ------------------------------------------------------------------------------------------------ C ABI

def test_symbols_are_declared_with_the_signatures_hip_binds():
    from ctrlora_amd import hip
    from tests.test_capi_symbols import _cls, _header_decls
    decls = _header_decls()
    P, L, I = ctypes.c_void_p, ctypes.c_long, ctypes.c_int
    want = {"cl_adamw_dev_groups": ("int", [P, P, P, P, L, P, I, P, P, P, P]), "cl_lr_schedule": ("int", [P, I, P, I, P, P])}
    cmap = {P: "ptr", L: "long", I: "int"}
    for name, (ret, sig) in want.items():
        assert name in decls and name in hip.EXPORTED, name
        assert decls[name][0] == ret and hip._SIGS[name] == sig
        assert [_cls(a) for a in decls[name][1]] == [cmap[s] for s in sig], name
    assert [a.split()[-1].lstrip("*") for a in decls["cl_adamw_dev_groups"][1]] == \
        ["p", "g", "m", "v", "n", "hyper_table", "ngroups", "chunk_group", "step", "clip", "stream"]
    assert [a.split()[-1].lstrip("*") for a in decls["cl_lr_schedule"][1]] == ["hyper_table", "ngroups", "lr_table", "T", "step", "stream"]
    assert "const unsigned char* chunk_group" in decls["cl_adamw_dev_groups"][1] and "const float* g" in decls["cl_adamw_dev_groups"][1]
    hdr = open(os.path.join(ROOT, "include", "ctrlora_hip.h")).read()
    assert "#define CL_ABI_VERSION 7" in hdr
    doc = hdr[:hdr.index("int cl_adamw_dev_groups")]
    doc = doc[doc.rindex("/*"):]
    assert "added in ABI 7 (compatible)" in doc and "Refused" in doc and "clamped" in doc
    ew = " ".join(open(os.path.join(ROOT, "ctrlora_amd", "csrc", "elementwise.h")).read().split())
    assert "EW_EMA_UPDATE, EW_SWAP, EW_ADAMW_DEV_GROUPS, EW_LR_SCHEDULE };" in ew and ew.count("enum {") == 1, \
        "new records are appended, none renumbered"
    ids = [s.split("=")[0].strip() for s in ew[ew.index("enum {") + 6:ew.index("};")].split(",")]
    assert "EW_GEGLU_FWD = 1" in ew and ids.index("EW_SWAP") + 1 == 41 and ids.index("EW_ADAMW_DEV_GROUPS") + 1 == 42 and \
        ids.index("EW_LR_SCHEDULE") + 1 == 43 == len(ids), "the numbers tests/test_gpu_optim_groups.py reads the records by"


def test_host_side_refusals_launch_nothing():
    """CL_EINVAL (1) with host addresses and no GPU: every refusal is decided before anything is launched."""
    from ctrlora_amd import hip
    L = hip.lib()
    assert L.cl_abi_version() == 7
    mem = (ctypes.c_float * 256)()
    p = ctypes.addressof(mem)
    N = None
    G, S = L.cl_adamw_dev_groups, L.cl_lr_schedule
    calls = {
        "null p": G(N, p, p, p, 64, p, 2, p, p, N, N), "null g": G(p, N, p, p, 64, p, 2, p, p, N, N), "null m": G(p, p, N, p, 64, p, 2, p, p, N, N),
        "null v": G(p, p, p, N, 64, p, 2, p, p, N, N), "null table": G(p, p, p, p, 64, N, 2, p, p, N, N), "null map": G(p, p, p, p, 64, p, 2, N, p, N, N),
        "null step": G(p, p, p, p, 64, p, 2, p, N, N, N), "n = 0": G(p, p, p, p, 0, p, 2, p, p, N, N), "n < 0": G(p, p, p, p, -64, p, 2, p, p, N, N),
        "n = 63": G(p, p, p, p, 63, p, 2, p, p, N, N), "n = 65": G(p, p, p, p, 65, p, 2, p, p, N, N), "n = 96": G(p, p, p, p, 96, p, 2, p, p, N, N),
        "G = 0": G(p, p, p, p, 64, p, 0, p, p, N, N), "G = 9": G(p, p, p, p, 64, p, 9, p, p, N, N), "G < 0": G(p, p, p, p, 64, p, -1, p, p, N, N),
        "null everything, n = 0": G(N, N, N, N, 0, N, 1, N, N, N, N), "clip given, n = 65": G(p, p, p, p, 65, p, 2, p, p, p, N),
        "sched null table": S(N, 2, p, 3, p, N), "sched null lr": S(p, 2, N, 3, p, N), "sched null step": S(p, 2, p, 3, N, N),
        "sched T = 0": S(p, 2, p, 0, p, N), "sched T < 0": S(p, 2, p, -1, p, N), "sched G = 0": S(p, 0, p, 3, p, N), "sched G = 9": S(p, 9, p, 3, p, N),
    }
    wrong = {k: v for k, v in calls.items() if v != 1}
    assert not wrong, wrong
    out = (ctypes.c_int * 8)(*([7] * 8))
    assert L.cl_debug_ew_last_launch(out) == 0 and list(out) == [0] * 8
    assert all(v == 0.0 for v in mem)
