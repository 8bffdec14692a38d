"""EMA of the fine-tuned weights, the parts that need no GPU: the model's construction and state dict, ModelEma against the
reference's fixture, the Trainer's host update against a hand-written loop, seeding on load, ema_scope on CPU modules, the
extraction tool, the scripts' flags, the C ABI's declarations and host-side refusals, and -- through the recording stand-in
for the library -- what FusedAdamW launches with the EMA attached."""
import ctypes
import importlib.util
import os
from types import SimpleNamespace

import pytest
import torch

from tests import ema_ref as E
from tests.util import ROOT

FLAGS = [dict(), dict(norm_trainable=False), dict(zero_trainable=False), dict(norm_trainable=False, zero_trainable=False),
         dict(ft_with_lora=False)]
FLAG_IDS = ["default", "norm-frozen", "zero-frozen", "both-frozen", "full"]


def _model(ema=True, decay=0.9999, config="ctrlora_finetune_sd15_rank128.yaml", **cn):
    import bench

    def mutate(p):
        if ema:
            p.update(use_ema=True, ema_decay=decay)
        p["control_stage_config"]["params"].update(cn)
    m = bench.build_model(config, 0, tiny=True, mutate=mutate)
    if ema:
        m.reseed_ema()          # build_model re-draws the zero-initialised tensors after construction, without a load
    return m


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------ construction, state dict

@pytest.mark.parametrize("cn", FLAGS, ids=FLAG_IDS)
def test_use_ema_adds_exactly_the_shadow_keys(cn):
    off, on = _model(False, **cn), _model(True, **cn)
    k_off, k_on = list(off.state_dict()), list(on.state_dict())
    names = on.trainable_names()
    assert names == off.trainable_names() and len(names) > 0
    want = ["model_ema.decay", "model_ema.num_updates"] + ["model_ema." + ("control_model." + n).replace(".", "") for n in names]
    assert k_on == k_off + want, "the key list gains exactly the EMA's buffers, in trainable_names() order"
    assert "model_ema" not in dict(off.named_children()) and off.use_ema is False and on.use_ema is True
    sd = on.state_dict()
    assert sd["model_ema.decay"].dtype == torch.float32 and sd["model_ema.decay"].shape == ()
    assert float(sd["model_ema.decay"]) == float(torch.tensor(0.9999, dtype=torch.float32))
    assert sd["model_ema.num_updates"].dtype == torch.int and int(sd["model_ema.num_updates"]) == 0
    params = dict(on.control_model.named_parameters())
    for n in names:
        s = sd["model_ema." + ("control_model." + n).replace(".", "")]
        assert s.dtype == torch.float32 and E.same_bits(s, params[n]), n
    for k in k_off:
        assert torch.equal(sd[k], off.state_dict()[k]), k       # one seed, one model: nothing else changes


def test_refusals_at_construction():
    with pytest.raises(NotImplementedError, match="fine-tuning only"):
        _model(True, config="ctrlora_pretrain_sd15_9tasks_rank128.yaml")
    with pytest.raises(ValueError, match="ema_decay"):
        _model(True, decay=1.5)
    import bench
    for bad in (dict(parameterization="x0"), dict(learn_logvar=True)):
        with pytest.raises(NotImplementedError):
            bench.build_model("ctrlora_finetune_sd15_rank128.yaml", 0, tiny=True, mutate=lambda p: p.update(use_ema=True, **bad))


# ------------------------------------------------------------------------------------------------ ModelEma against the fixture

def _toy(run):
    toy = torch.nn.Module()
    for name, value in run["init"].items():
        mod, leaf = toy, name
        if "." in name:
            head, leaf = name.split(".")
            if not hasattr(toy, head):
                toy.add_module(head, torch.nn.Module())
            mod = getattr(toy, head)
        mod.register_parameter(leaf, torch.nn.Parameter(value.clone(), requires_grad=name != "frozen"))
    return toy


@pytest.mark.parametrize("name", ["defaults", "no_warmup", "crossing"])
def test_model_ema_forward_matches_the_reference_bit_for_bit(name):
    from ldm.modules.ema import ModelEma
    run = E.load_fixture()[name]
    cfg = run["cfg"]
    toy = _toy(run)
    ema = ModelEma(toy, decay=cfg["decay"], use_num_updates=cfg["use_num_updates"])
    if cfg["preset"] is not None:
        ema.num_updates.fill_(cfg["preset"])
    assert ema.m_name2s_name == run["names"] and "frozen" not in ema.m_name2s_name
    assert set(dict(ema.named_buffers())) == {"decay", "num_updates"} | set(run["names"].values())
    for k in range(12):
        with torch.no_grad():
            for n, p in toy.named_parameters():
                p.copy_(run["params"][k][n])          # the frozen one moves too, and is ignored
        ema(toy)
        assert int(ema.num_updates) == run["num_updates"][k]
        for key, want in run["shadows"][k].items():
            assert E.same_bits(ema._buffers[key], want), (name, k, key)
    # the same through (name, tensor) pairs
    ema2 = ModelEma([(n, v) for n, v in run["init"].items() if n != "frozen"], decay=cfg["decay"], use_num_updates=cfg["use_num_updates"])
    if cfg["preset"] is not None:
        ema2.num_updates.fill_(cfg["preset"])
    ema2(run["params"][0])
    assert all(E.same_bits(ema2._buffers[key], want) for key, want in run["shadows"][0].items())


def test_model_ema_keeps_litemas_other_meanings():
    from ldm.modules.ema import ModelEma
    run = E.load_fixture()["defaults"]
    toy = _toy(run)
    ema = ModelEma(toy)
    with pytest.raises(ValueError):
        ModelEma(toy, decay=1.1)
    with torch.no_grad():
        for p in toy.parameters():
            p.add_(1.0)
    ema(toy)
    moved = {n: p.detach().clone() for n, p in toy.named_parameters()}
    trainable = [p for p in toy.parameters() if p.requires_grad]
    ema.store(trainable)
    ema.copy_to(toy)
    for n, p in toy.named_parameters():
        assert torch.equal(p, ema.shadows()[n] if n != "frozen" else moved[n])
        assert n == "frozen" or not torch.equal(p, moved[n])
    ema.restore(trainable)
    assert all(E.same_bits(p, moved[n]) for n, p in toy.named_parameters())
    assert int(ema.num_updates) == 1
    ema.reset_num_updates()
    assert int(ema.num_updates) == 0 and ema.num_updates.dtype == torch.int
    ema.seed(toy)
    assert all(E.same_bits(ema.shadows()[n], moved[n]) for n in ema.shadows()) and not ema.touched
    ema.set_decay(0.5)
    assert float(ema.decay) == float(torch.tensor(0.9999)), "a host change waits for sync()"
    ema.sync()
    assert float(ema.decay) == 0.5


# ------------------------------------------------------------------------------------------------ Trainer, host update

class _Small(torch.nn.Module):
    def __init__(self, ema=True):
        super().__init__()
        from ldm.modules.ema import ModelEma
        torch.manual_seed(3)
        self.net = torch.nn.Sequential(torch.nn.Linear(6, 16), torch.nn.Tanh(), torch.nn.Linear(16, 1))
        self.net[0].bias.requires_grad_(False)
        if ema:
            self.model_ema = ModelEma([("net." + n, p) for n, p in self.net.named_parameters() if p.requires_grad], decay=0.9)

    def training_step(self, batch, batch_idx):
        x, y = batch
        return ((self.net(x) - y) ** 2).mean()

    def configure_optimizers(self):
        return torch.optim.AdamW([p for p in self.net.parameters() if p.requires_grad], lr=1e-2)


def _data(n):
    g = torch.Generator().manual_seed(9)
    return [(torch.randn(5, 6, generator=g), torch.randn(5, 1, generator=g)) for _ in range(n)]


@pytest.mark.parametrize("acc", [1, 2])
def test_trainer_updates_once_per_optimizer_step_like_a_hand_written_loop(acc, tmp_path):
    from ctrlora_amd.trainer import Trainer
    m = _Small(ema=False).train()
    opt = m.configure_optimizers()
    names = [n for n, p in m.named_parameters() if p.requires_grad]
    shadows = {n: p.detach().numpy().copy() for n, p in m.named_parameters() if p.requires_grad}
    opt.zero_grad()
    u = 0
    for i, batch in enumerate(_data(4 * acc)):
        (m.training_step(batch, i) / acc).backward()
        if (i + 1) % acc == 0:
            opt.step()
            opt.zero_grad()
            u += 1
            params = dict(m.named_parameters())
            shadows = {n: E.update(shadows[n], params[n].detach().numpy(), 0.9, u) for n in names}
    got = _Small().train()
    tr = Trainer(max_steps=4, accumulate_grad_batches=acc, device="cpu", default_root_dir=str(tmp_path), log_every_n_steps=1)
    tr.fit(got, _data(4 * acc))
    assert tr.global_step == 4 and int(got.model_ema.num_updates) == 4, "num_updates counts optimizer steps, not micro-batches"
    for n in names:
        assert torch.equal(dict(got.named_parameters())[n], dict(m.named_parameters())[n]), "the EMA does not touch training"
        assert E.same_bits(got.model_ema.shadows()[n], shadows[n]), n
        assert not E.same_bits(got.model_ema.shadows()[n], dict(got.named_parameters())[n])
    assert set(got.model_ema.shadows()) == set(names) and "net.0.bias" not in names
    # without a model_ema the loop is what it was
    plain = _Small(ema=False)
    Trainer(max_steps=4, accumulate_grad_batches=acc, device="cpu", default_root_dir=str(tmp_path), log_every_n_steps=1).fit(plain, _data(4 * acc))
    assert all(torch.equal(a, b) for a, b in zip(plain.net.state_dict().values(), m.net.state_dict().values()))


# ------------------------------------------------------------------------------------------------ seeding, loading, scope

def test_load_state_dict_reseeds_or_restores(capsys):
    m = _model(True, decay=0.9)
    names = m.trainable_names()
    P = lambda: m._ema_named_params()
    m.model_ema(m)
    m.model_ema(m)
    assert int(m.model_ema.num_updates) == 2 and m.model_ema.touched
    with_ema = {k: v.clone() for k, v in m.state_dict().items()}
    without = {k: v.clone() + (0.25 if "lora_layer" in k else 0.0) for k, v in with_ema.items() if not k.startswith("model_ema.")}
    # a source without model_ema.* keys (an --sd_ckpt / --cn_ckpt style load): shadows == the loaded parameters, count 0
    res = m.load_state_dict(without, strict=False)
    assert sorted(res.missing_keys) == sorted(k for k in with_ema if k.startswith("model_ema.")) and not res.unexpected_keys
    assert int(m.model_ema.num_updates) == 0 and not m.model_ema.touched
    assert "the average of 2 updates is discarded" in capsys.readouterr().out, "a re-seed that throws updates away says so"
    sh = m.model_ema.shadows()
    assert list(sh) == ["control_model." + n for n in names]
    assert all(E.same_bits(sh[n], p) and E.same_bits(p, without[n]) for n, p in P().items())
    with pytest.raises(RuntimeError, match="Missing key.*model_ema"):
        m.load_state_dict(without, strict=True)
    # a source that carries them: restored like any buffer
    for k in with_ema:
        if k.startswith("model_ema.control_model"):
            with_ema[k] = with_ema[k] + 1.0
    with_ema["model_ema.num_updates"] = torch.tensor(41, dtype=torch.int)
    m.load_state_dict(with_ema, strict=True)
    assert int(m.model_ema.num_updates) == 41 and m.model_ema.touched
    sd = m.state_dict()
    assert all(torch.equal(sd[k], with_ema[k]) for k in with_ema)
    # and a model without EMA refuses the checkpoint strictly, as torch reports it
    with pytest.raises(RuntimeError, match="Unexpected key.*model_ema"):
        _model(False).load_state_dict(with_ema, strict=True)


@pytest.mark.parametrize("raises", [False, True])
def test_ema_scope_on_cpu_swaps_and_restores(raises):
    m = _model(True, decay=0.5)
    with torch.no_grad():
        for p in m._ema_named_params().values():
            p.add_(0.125)
    m.model_ema(m)
    before = {n: p.detach().clone() for n, p in m._ema_named_params().items()}
    shadows = {n: s.clone() for n, s in m.model_ema.shadows().items()}
    assert not any(E.same_bits(before[n], shadows[n]) for n in before if before[n].abs().max() > 0)

    class Boom(Exception):
        pass
    try:
        with m.ema_scope("test"):
            assert m.model_ema.in_scope
            assert all(E.same_bits(p, shadows[n]) for n, p in m._ema_named_params().items()), "inside: the shadows"
            if raises:
                raise Boom()
    except Boom:
        assert raises
    assert not m.model_ema.in_scope
    assert all(E.same_bits(p, before[n]) for n, p in m._ema_named_params().items()), "after: the original bits"
    assert all(E.same_bits(s, shadows[n]) for n, s in m.model_ema.shadows().items())
    with _model(False).ema_scope():          # use_ema off: a no-op, like the reference
        pass


# ------------------------------------------------------------------------------------------------ tool_extract_weights

def test_extraction_skips_the_shadows_and_ema_takes_them(tmp_path):
    X = _script("tool_extract_weights")
    m = _model(True, decay=0.5)
    with torch.no_grad():
        for p in m._ema_named_params().values():
            p.add_(0.5)
    m.model_ema(m)
    ckpt = {k: v.clone() for k, v in m.state_dict().items()}
    plain = {k: v for k, v in ckpt.items() if not k.startswith("model_ema.")}
    lora, lora_plain = X.extract_lora(ckpt), X.extract_lora(plain)
    assert list(lora) == list(lora_plain) and len(lora) == len(m.trainable_names()) == 246
    assert list(X.extract_control(ckpt)) == list(X.extract_control(plain))
    assert not any(k.startswith("model_ema.") for k in list(lora) + list(X.extract_control(ckpt)))
    ck_path, out_path = str(tmp_path / "last.ckpt"), str(tmp_path / "lora_ema.ckpt")
    torch.save({"state_dict": ckpt}, ck_path)
    X.main(["-t", "lora", "--ckpt", ck_path, "--save_path", out_path, "--ema"])
    got = torch.load(out_path, map_location="cpu", weights_only=False)
    assert list(got) == list(lora)
    for k, v in got.items():
        assert v.shape == ckpt[k].shape and torch.equal(v, ckpt["model_ema." + k.replace(".", "")]), k
    assert sum(int(not torch.equal(got[k], lora[k])) for k in got) > 200, "the averages are not the weights"
    # --ema on a checkpoint without shadows names the first missing key
    torch.save({"state_dict": plain}, ck_path)
    first = "model_ema." + next(iter(lora)).replace(".", "")
    with pytest.raises(SystemExit, match=first):
        X.main(["-t", "lora", "--ckpt", ck_path, "--save_path", out_path, "--ema"])
    # and -t control --ema wants a shadow for every control_model tensor: the frozen ones have none
    torch.save({"state_dict": ckpt}, ck_path)
    with pytest.raises(SystemExit, match="model_ema"):
        X.main(["-t", "control", "--ckpt", ck_path, "--save_path", out_path, "--ema"])
    with pytest.raises(SystemExit):
        X.main(["-t", "lora", "--ckpt", ck_path, "--save_path", out_path, "--ema", "--from_base"])
    # the dispatch is the reference's: -t control writes the control file with or without --from_base
    X.main(["-t", "control", "--ckpt", ck_path, "--save_path", out_path, "--from_base"])
    got = torch.load(out_path, map_location="cpu", weights_only=False)
    assert list(got) == list(X.extract_control(plain)) and all(torch.equal(got[k], ckpt[k]) for k in got)


# ------------------------------------------------------------------------------------------------ scripts' flags

def test_ema_decay_flag_on_the_finetune_script_only(capsys):
    train = _script("train_ctrlora_finetune")
    p = train.get_parser()
    base = ["--dataroot", "d", "--config", "c", "--sd_ckpt", "s", "--cn_ckpt", "n"]
    assert p.parse_args(base).ema_decay == 0.0 and train.ema_model_params(0.0) == {}
    a = p.parse_args(base + ["--ema_decay", "0.999", "--graph", "--gradacc", "2", "--latent_cache", "x", "--grad_clip", "1.0"])
    assert a.ema_decay == 0.999 and a.graph and a.gradacc == 2
    assert train.ema_model_params(a.ema_decay) == dict(use_ema=True, ema_decay=0.999)
    assert p.parse_args(base + ["--ema_decay", "1.0"]).ema_decay == 1.0
    for bad in ("1.5", "-0.1"):
        with pytest.raises(SystemExit):
            p.parse_args(base + ["--ema_decay", bad])
    assert "--ema_decay" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        _script("train_ctrlora_pretrain").get_parser().parse_args(base + ["--ema_decay", "0.9"])


def test_create_model_takes_the_flag_and_init_weights_reseeds(tmp_path):
    import yaml
    from cldm.model import create_model
    train = _script("train_ctrlora_finetune")
    with open(os.path.join(ROOT, "configs", "ctrlora_finetune_sd15_rank128.yaml")) as f:
        tree = yaml.safe_load(f)
    p = tree["model"]["params"]
    p["first_stage_config"] = {"target": "torch.nn.Identity"}
    p["cond_stage_config"] = {"target": "torch.nn.Identity"}
    for k in ("control_stage_config", "unet_config"):
        p[k]["params"].update(model_channels=32, context_dim=64, num_heads=4)
    p["control_stage_config"]["params"]["lora_rank"] = 8
    cfg = str(tmp_path / "narrow.yaml")
    with open(cfg, "w") as f:
        yaml.safe_dump(tree, f)
    assert not hasattr(create_model(cfg), "model_ema")
    m = create_model(cfg, params=train.ema_model_params(0.99))
    assert m.use_ema and float(m.model_ema.decay) == float(torch.tensor(0.99))
    assert all(E.same_bits(m.model_ema.shadows()[n], q) for n, q in m._ema_named_params().items()), "seeded after the fill"
    sd = {k: v + 0.5 for k, v in m.state_dict().items() if k.startswith("model.diffusion_model.")}
    cn = {k: v - 0.5 for k, v in m.state_dict().items() if k.startswith("control_model.")}
    m.model_ema(m)
    train.init_weights(m, sd, cn, report_dir=None)
    assert int(m.model_ema.num_updates) == 0
    params = m._ema_named_params()
    assert all(E.same_bits(m.model_ema.shadows()[n], q) for n, q in params.items()), "the average starts at the loaded weights"
    moved = [n for n, q in params.items() if "lora" not in n and torch.equal(q, cn[n])]
    assert moved, "the base ControlNet's trained tensors were loaded"


def test_sample_script_use_ema_flag_and_refusals():
    sample = _script("sample")
    p = sample.get_parser()
    base = ["--dataroot", "d", "--config", "c", "--ckpt", "k", "--save_dir", "s"]
    assert p.parse_args(base).use_ema is False and p.parse_args(base + ["--use_ema"]).use_ema is True
    on, off = _model(True), _model(False)
    assert "use_ema: true" in sample.ema_refusal(off, off.state_dict())
    why = sample.ema_refusal(on, off.state_dict())
    assert "model_ema.decay" in why and "248" in why
    assert sample.ema_refusal(on, on.state_dict()) is None


# ------------------------------------------------------------------------------------------------ C ABI

def test_symbols_are_declared_with_the_signatures_hip_binds():
    from ctrlora_amd import hip
    from tests.test_capi_symbols import _cls, _header_decls
    decls = _header_decls()
    P, L = ctypes.c_void_p, ctypes.c_long
    want = {"cl_ema_update": ("int", [P, P, L, P, P, P]), "cl_swap": ("int", [P, P, L, P])}
    cmap = {P: "ptr", L: "long"}
    for name, (ret, sig) in want.items():
        assert name in decls and name in hip.EXPORTED, name
        assert decls[name][0] == ret and hip._SIGS[name] == sig
        assert [_cls(a) for a in decls[name][1]] == [cmap[s] for s in sig], name
    assert [a.split()[-1].lstrip("*") for a in decls["cl_ema_update"][1]] == ["shadow", "p", "n", "decay", "num_updates", "stream"]
    assert "const float* p" in decls["cl_ema_update"][1] and "const int* num_updates" in decls["cl_ema_update"][1]
    hdr = open(os.path.join(ROOT, "include", "ctrlora_hip.h")).read()
    assert "#define CL_ABI_VERSION 7" in hdr
    doc = hdr[:hdr.index("int cl_ema_update")]
    assert "added in ABI 7 (compatible)" in doc[doc.rindex("/*"):], "the additions are marked compatible where they are declared"
    ew = open(os.path.join(ROOT, "ctrlora_amd", "csrc", "elementwise.h")).read().replace("\n", " ")
    ew = " ".join(ew.split())
    assert "EW_ADAMW_DEV_CLIP, EW_EMA_UPDATE, EW_SWAP, EW_ADAMW_DEV_GROUPS, EW_LR_SCHEDULE };" in ew, "new records are appended, none renumbered"
    ids = [s.split("=")[0].strip() for s in ew[ew.index("enum {") + 6:ew.index("};")].split(",")]
    assert ids[0] == "EW_GEGLU_FWD" and ids.index("EW_ADAMW_DEV_CLIP") + 1 == 39 and ids.index("EW_EMA_UPDATE") + 1 == 40 and \
        ids.index("EW_SWAP") + 1 == 41, "one enum counted from 1: the numbers cl_debug_ew_last_launch reports"


def test_abi_is_still_7_and_host_side_refusals_launch_nothing():
    from ctrlora_amd import hip
    L = hip.lib()
    assert L.cl_abi_version() == 7
    mem = (ctypes.c_float * 64)()
    p = ctypes.addressof(mem)
    N = None
    calls = {
        "ema null shadow": L.cl_ema_update(N, p + 128, 4, p, p, N), "ema null p": L.cl_ema_update(p, N, 4, p, p, N),
        "ema null decay": L.cl_ema_update(p, p + 128, 4, N, p, N), "ema null count": L.cl_ema_update(p, p + 128, 4, p, N, N),
        "ema null decay, n = 0": L.cl_ema_update(p, p + 128, 0, N, p, N), "ema n < 0": L.cl_ema_update(p, p + 128, -1, p, p, N),
        "ema off 4 bytes": L.cl_ema_update(p + 2, p + 128, 4, p, p, N), "ema overlap": L.cl_ema_update(p, p + 8, 4, p, p, N),
        "swap null a": L.cl_swap(N, p, 4, N), "swap null b": L.cl_swap(p, N, 4, N), "swap n < 0": L.cl_swap(p, p + 128, -1, N),
        "swap overlap": L.cl_swap(p, p + 8, 4, N), "swap off 4 bytes": L.cl_swap(p, p + 130, 4, N),
    }
    wrong = {k: v for k, v in calls.items() if v != 1}
    assert not wrong, wrong
    fine = {"ema n = 0": L.cl_ema_update(N, N, 0, p, p, N), "swap n = 0": L.cl_swap(N, N, 0, N), "swap a == b": L.cl_swap(p, p, 64, N)}
    assert not {k: v for k, v in fine.items() if v != 0}
    out = (ctypes.c_int * 8)(*([7] * 8))
    assert L.cl_debug_ew_last_launch(out) == 0 and list(out) == [0] * 8
    assert all(v == 0.0 for v in mem)


# ------------------------------------------------------------------------------------------------ what FusedAdamW launches

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


def test_fused_adamw_launches_with_and_without_the_ema(rec):
    from ctrlora_amd.train import FusedAdamW
    from ldm.modules.ema import ModelEma
    exs = [_fake_ex(40, 1), _fake_ex(24, 2)]
    opt = FusedAdamW([torch.nn.Parameter(ex.tr.flat) for ex in exs], exs, lr=1e-3)
    assert opt.ema is None
    opt.step()
    today = ["cl_tick", "cl_adamw_dev", "cl_adamw_dev"]
    assert rec.names() == today, "without the EMA the step launches exactly what it did"
    ema = ModelEma([("a", exs[0].tr.flat), ("b", exs[1].tr.flat)], decay=0.9)
    flats = [torch.zeros_like(ex.tr.flat) for ex in exs]
    opt.attach_ema(ema, flats)
    for clip, adamw in ((None, "cl_adamw_dev"), (1.0, "cl_adamw_dev_clip")):
        opt.max_grad_norm = clip
        rec.clear()
        opt.step()
        names = [n for n in rec.names() if n != "cl_grad_norm_scratch_floats"]
        assert names == ["cl_grad_norm"] * bool(clip) + ["cl_tick", "cl_tick", adamw, "cl_ema_update", adamw, "cl_ema_update"], names
        ticks = rec.of("cl_tick")
        assert [t[0] for t in ticks] == [opt._step_dev.data_ptr(), ema.num_updates.data_ptr()], "one tick each per optimizer step"
        for a, ex, f in zip(rec.of("cl_ema_update"), exs, flats):
            assert a[:5] == (f.data_ptr(), ex.tr.flat.data_ptr(), ex.tr.flat.numel(), ema.decay.data_ptr(), ema.num_updates.data_ptr())
    # a decay change reaches the device tensor with sync_hyper(), at the next step
    ema.set_decay(0.25)
    assert float(ema.decay) == float(torch.tensor(0.9))
    opt.step()
    assert float(ema.decay) == 0.25
    # inside the scope the step refuses, and launches nothing
    ema.in_scope = True
    rec.clear()
    with pytest.raises(RuntimeError, match="ema_scope"):
        opt.step()
    assert rec.names() == []
    ema.in_scope = False
    # without the warm-up the count is not ticked: it stays at -1
    ema2 = ModelEma([("a", exs[0].tr.flat), ("b", exs[1].tr.flat)], decay=0.9, use_num_updates=False)
    opt.attach_ema(ema2, flats)
    opt.max_grad_norm = None
    rec.clear()
    opt.step()
    assert rec.names() == ["cl_tick", "cl_adamw_dev", "cl_ema_update", "cl_adamw_dev", "cl_ema_update"]
