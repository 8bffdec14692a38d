"""Latent cache (ctrlora_amd/latent_cache.py, datasets/cached_latents.py, ControlLDM.get_input's cached branch), CPU only:
builder -> dataset -> items round trip with a stub encoder of known moments, the refusals, the cached get_input against
scale * (mean + std * randn) under the same seed (torch form of the pair op), the prompt drop-out stream, the parser."""
import importlib.util
import json
import os
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests.util import ROOT


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _make_root(path, n=5, size=(8, 16), odd=None):
    """A CustomDataset directory of n PNG pairs of `size` (record `odd` gets another size)."""
    from PIL import Image
    os.makedirs(path / "source"), os.makedirs(path / "target")
    rng = np.random.RandomState(1)
    with open(path / "prompt.json", "w") as f:
        for i in range(n):
            hw = (16, 16) if i == odd else size
            for d in ("source", "target"):
                Image.fromarray(rng.randint(0, 256, hw + (3,), dtype=np.uint8)).save(path / d / f"{i:04d}.png")
            f.write(json.dumps({"source": f"source/{i:04d}.png", "target": f"target/{i:04d}.png", "prompt": f"prompt {i}"}) + "\n")
    return str(path)


def _stub_moments(x):
    """Known moments of an NCHW batch: 4 channels at half resolution."""
    mean = torch.cat([x, x[:, :1] * 0.5], 1)[:, :, ::2, ::2].contiguous()
    return mean, 0.25 + 0.5 * mean.abs()


def _stub_encode(x):
    assert x.dim() == 4 and x.shape[1] == 3 and x.dtype == torch.float32 and x.is_contiguous()
    mean, std = _stub_moments(x)
    return types.SimpleNamespace(mean=mean, std=std)


def _nchw(a):
    return torch.from_numpy(a)[None].permute(0, 3, 1, 2).contiguous().float()


def test_builder_dataset_round_trip_with_known_moments(tmp_path, monkeypatch):
    from ctrlora_amd import latent_cache as LC
    from datasets.cached_latents import CachedLatentDataset
    from datasets.custom_dataset import CustomDataset
    root, out = _make_root(tmp_path / "data"), str(tmp_path / "cache")
    live = CustomDataset(root, drop_rate=0)
    renamed = []
    real_replace = os.replace
    monkeypatch.setattr(os, "replace", lambda a, b: (renamed.append(os.path.basename(b)), real_replace(a, b))[1])
    meta = LC.build_cache(live, _stub_encode, out, bs=2, engine_dtype="fp32", fingerprint="abc")      # 5 items: 2 + 2 + 1
    assert renamed == [LC.TARGET, LC.HINT, LC.META], "meta.json must be renamed into place last"
    assert sorted(os.listdir(out)) == sorted([LC.TARGET, LC.HINT, LC.META]), "temporary files left behind"
    assert meta == json.load(open(os.path.join(out, LC.META)))
    assert (meta["N"], meta["latent_shape"], meta["engine_dtype"], meta["first_stage_sha256"]) == (5, [4, 4, 8], "fp32", "abc")
    assert meta["records"] == live.data and meta["format_version"] == LC.FORMAT_VERSION
    ds = CachedLatentDataset(root, out, drop_rate=0.0)
    assert len(ds) == 5 and isinstance(ds.target, np.memmap) and isinstance(ds.hint, np.memmap)
    assert ds.target.shape == ds.hint.shape == (5, 8, 4, 8) and ds.target.dtype == np.float32
    for i in (0, 3, 4):                                                   # index order, across the batch boundaries
        it, ref = ds[i], live[i]
        assert set(it) == {"jpg_moments", "hint_moments", "txt"} and it["txt"] == f"prompt {i}"
        for key, img in (("jpg_moments", ref["jpg"]), ("hint_moments", ref["hint"])):
            mean, std = _stub_moments(_nchw(img))
            assert it[key].dtype == np.float32 and it[key].shape == (8, 4, 8) and type(it[key]) is np.ndarray
            assert np.array_equal(it[key][:4], mean[0].numpy()) and np.array_equal(it[key][4:], std[0].numpy())
    assert not np.array_equal(ds[0]["jpg_moments"], ds[0]["hint_moments"])


def test_a_half_written_cache_does_not_load_and_a_failed_rebuild_keeps_the_old_cache(tmp_path, monkeypatch):
    from ctrlora_amd import latent_cache as LC
    from datasets.cached_latents import CachedLatentDataset
    from datasets.custom_dataset import CustomDataset
    root, out = _make_root(tmp_path / "data"), str(tmp_path / "cache")
    live = CustomDataset(root, drop_rate=0)
    LC.build_cache(live, _stub_encode, out, bs=2, fingerprint="first")
    before = CachedLatentDataset(root, out)[4]
    calls = []

    def failing(x):
        calls.append(1)
        if len(calls) > 3:
            raise RuntimeError("encoder died")
        return _stub_encode(x)
    with pytest.raises(RuntimeError, match="encoder died"):
        LC.build_cache(live, failing, out, bs=2, fingerprint="second")    # a rebuild over the old cache that dies half way
    assert not [f for f in os.listdir(out) if ".tmp" in f]
    ds = CachedLatentDataset(root, out)                                   # the old cache is as it was
    assert ds.meta["first_stage_sha256"] == "first" and np.array_equal(ds[4]["hint_moments"], before["hint_moments"])
    del ds
    # a build killed between the renames: the arrays are in place, meta.json is not -> nothing loads
    real_replace = os.replace

    def dying(a, b):
        if b.endswith(LC.META):
            raise KeyboardInterrupt
        real_replace(a, b)
    monkeypatch.setattr(os, "replace", dying)
    with pytest.raises(KeyboardInterrupt):
        LC.build_cache(live, _stub_encode, out, bs=2, fingerprint="third")
    monkeypatch.setattr(os, "replace", real_replace)
    assert not os.path.exists(os.path.join(out, LC.META)) and os.path.exists(os.path.join(out, LC.TARGET))
    with pytest.raises(LC.LatentCacheError, match="meta.json not found"):
        CachedLatentDataset(root, out)
    with pytest.raises(LC.LatentCacheError, match="meta.json not found"):
        LC.open_cache(str(tmp_path / "nowhere"))
    # temporary files of a killed build (another process id) are swept by the next build
    for k in (LC.TARGET, LC.META):
        open(os.path.join(out, k + ".tmp99999"), "w").close()
    LC.build_cache(live, _stub_encode, out, bs=2, fingerprint="fourth")
    assert sorted(os.listdir(out)) == sorted([LC.TARGET, LC.HINT, LC.META])
    assert CachedLatentDataset(root, out).meta["first_stage_sha256"] == "fourth"


def test_refusals_name_what_differs(tmp_path):
    from ctrlora_amd import latent_cache as LC
    from datasets.cached_latents import CachedLatentDataset
    from datasets.custom_dataset import CustomDataset
    # images of differing sizes
    mixed = _make_root(tmp_path / "mixed", odd=3)
    with pytest.raises(LC.LatentCacheError, match=r"differing sizes.*record 3 \(target/0003.png"):
        LC.build_cache(CustomDataset(mixed, drop_rate=0), _stub_encode, str(tmp_path / "mixed_cache"), bs=2)
    assert not os.path.exists(tmp_path / "mixed_cache" / LC.META)
    # count and record list against prompt.json
    root, out = _make_root(tmp_path / "data"), str(tmp_path / "cache")
    LC.build_cache(CustomDataset(root, drop_rate=0), _stub_encode, out, bs=4, fingerprint="")
    lines = open(os.path.join(root, "prompt.json")).read().splitlines()
    with open(os.path.join(root, "prompt.json"), "w") as f:
        f.write("\n".join(lines[:4]) + "\n")
    with pytest.raises(LC.LatentCacheError, match="holds 5 items, prompt.json lists 4"):
        CachedLatentDataset(root, out)
    edited = lines[:1] + [lines[1].replace("prompt 1", "another prompt")] + lines[2:]
    with open(os.path.join(root, "prompt.json"), "w") as f:
        f.write("\n".join(edited) + "\n")
    with pytest.raises(LC.LatentCacheError, match="differs from prompt.json at record 1"):
        CachedLatentDataset(root, out)
    with open(os.path.join(root, "prompt.json"), "w") as f:
        f.write("\n".join(lines) + "\n")
    ds = CachedLatentDataset(root, out)
    # fingerprint of the first stage, and the engine dtype
    torch.manual_seed(0)
    m1, m2 = (types.SimpleNamespace(first_stage_model=nn.Conv2d(3, 8, 3)) for _ in range(2))
    assert LC.state_fingerprint(m1.first_stage_model) != LC.state_fingerprint(m2.first_stage_model)
    ds.meta["first_stage_sha256"] = LC.state_fingerprint(m1.first_stage_model)
    LC.check_model(ds.meta, m1, torch.float32)
    with pytest.raises(LC.LatentCacheError, match="another first_stage_model"):
        LC.check_model(ds.meta, m2, torch.float32)
    with pytest.raises(LC.LatentCacheError, match="encoded in fp32, training runs the engine in bf16"):
        LC.check_model(ds.meta, m1, torch.bfloat16)
    with torch.no_grad():
        m1.first_stage_model.bias[3] += 1e-6                              # one changed element is another model
    with pytest.raises(LC.LatentCacheError, match="another first_stage_model"):
        LC.check_model(ds.meta, m1, torch.float32)
    # an array that is not what meta.json describes
    del ds
    np.save(os.path.join(out, LC.HINT), np.zeros((5, 8, 4, 4), np.float32))
    with pytest.raises(LC.LatentCacheError, match="hint_moments.npy is float32"):
        CachedLatentDataset(root, out)


def test_train_script_flag_defaults_and_multigen_refusal(tmp_path):
    tool = _script("train_ctrlora_finetune")
    base = ["--dataroot", "d", "--config", "c.yaml", "--sd_ckpt", "s", "--cn_ckpt", "n"]
    a = tool.get_parser().parse_args(base)
    assert a.latent_cache is None
    assert (a.lr, a.bs, a.max_steps, a.gradacc, a.precision, a.drop_rate) == (1e-5, 1, 100000, 1, 32, 0.3)
    assert (a.img_logger_freq, a.ckpt_logger_freq, a.subset, a.multigen20m, a.save_memory, a.num_workers) == (1000, 1000, 0, False, False, None)
    b = tool.get_parser().parse_args(base + ["--latent_cache", "dir", "--multigen20m", "--task", "canny"])
    assert b.latent_cache == "dir"
    with pytest.raises(ValueError, match="--latent_cache cannot be combined with --multigen20m"):
        tool.build_dataloader(b, 1, 0)
    # with the flag, build_dataloader hands out the cached dataset; without it, CustomDataset as before
    from ctrlora_amd import latent_cache as LC
    from datasets.cached_latents import CachedLatentDataset
    from datasets.custom_dataset import CustomDataset
    root, out = _make_root(tmp_path / "data"), str(tmp_path / "cache")
    LC.build_cache(CustomDataset(root, drop_rate=0), _stub_encode, out, bs=4)
    args = tool.get_parser().parse_args(["--dataroot", root] + base[2:] + ["--latent_cache", out, "--bs", "2", "--num_workers", "0"])
    ds, loader = tool.build_dataloader(args, 1, 0)
    assert isinstance(ds, CachedLatentDataset) and ds.drop_rate == 0.3
    batch = next(iter(loader))
    assert batch["jpg_moments"].shape == batch["hint_moments"].shape == (2, 8, 4, 8) and batch["jpg_moments"].dtype == torch.float32
    assert len(batch["txt"]) == 2 and set(batch) == {"jpg_moments", "hint_moments", "txt"}
    args.latent_cache = None
    assert isinstance(tool.build_dataloader(args, 1, 0)[0], CustomDataset)


def test_prompt_dropout_stream_equals_custom_dataset(tmp_path):
    from ctrlora_amd import latent_cache as LC
    from datasets.cached_latents import CachedLatentDataset
    from datasets.custom_dataset import CustomDataset
    root, out = _make_root(tmp_path / "data"), str(tmp_path / "cache")
    LC.build_cache(CustomDataset(root, drop_rate=0), _stub_encode, out)
    order = [0, 3, 1, 4, 2] * 6
    np.random.seed(5)
    live = [CustomDataset(root, drop_rate=0.4)[i]["txt"] for i in order]
    state = np.random.get_state()[1].copy()
    np.random.seed(5)
    cached = [CachedLatentDataset(root, out, drop_rate=0.4)[i]["txt"] for i in order]
    assert cached == live and "" in live and any(live)
    assert np.array_equal(np.random.get_state()[1], state)               # the stream is left where CustomDataset leaves it


class _NoImages(dict):
    def __getitem__(self, k):
        assert k not in ("jpg", "hint"), f"the cached branch read batch[{k!r}]"
        return super().__getitem__(k)


def test_cached_get_input_draws_target_then_hint_bit_equal():
    from tests.test_training_scripts import _tiny_ldm
    model = _tiny_ldm(0)
    model.scale_factor = 0.18215
    g = torch.Generator().manual_seed(2)
    B, C, h, w = 3, 4, 5, 7                                              # odd sizes: per-sample count not a multiple of 4
    mom = [torch.cat([torch.randn(B, C, h, w, generator=g), torch.rand(B, C, h, w, generator=g) + 0.1], 1) for _ in range(2)]
    batch = _NoImages(jpg_moments=mom[0], hint_moments=mom[1], txt=["a", "", "c"])
    torch.manual_seed(7)
    z, cond = model.get_input(batch, model.first_stage_key)
    torch.manual_seed(7)
    e_x = torch.randn(B, C, h, w)
    e_h = torch.randn(B, C, h, w)                                         # target first, hint second
    sf = model.scale_factor
    assert torch.equal(z, sf * (mom[0][:, :C] + mom[0][:, C:] * e_x))
    assert torch.equal(cond["c_concat"][0], sf * (mom[1][:, :C] + mom[1][:, C:] * e_h))
    assert set(cond) == {"c_crossattn", "c_concat"} and cond["c_crossattn"] == [["a", "", "c"]]
    assert z.dtype == torch.float32 and z.shape == (B, C, h, w) and len(cond["c_concat"]) == 1
    # the posterior's own sample() under the same seed: the live path's arithmetic
    from ldm.modules.distributions.distributions import DiagonalGaussianDistribution
    torch.manual_seed(7)
    live = DiagonalGaussianDistribution(torch.cat([mom[0][:, :C], 2 * torch.log(mom[0][:, C:])], 1))
    live.std = mom[0][:, C:]
    assert torch.equal(z, model.get_first_stage_encoding(live))
    # bs (log_images): the first rows, drawn at the smaller shape
    torch.manual_seed(7)
    z2, cond2 = model.get_input(batch, model.first_stage_key, bs=2)
    torch.manual_seed(7)
    e_x2, e_h2 = torch.randn(2, C, h, w), torch.randn(2, C, h, w)
    assert torch.equal(z2, sf * (mom[0][:2, :C] + mom[0][:2, C:] * e_x2))
    assert torch.equal(cond2["c_concat"][0], sf * (mom[1][:2, :C] + mom[1][:2, C:] * e_h2)) and cond2["c_crossattn"] == [["a", ""]]
    # _hint_latent passes the 4-channel hint latent through untouched
    assert model._hint_latent(cond) is cond["c_concat"][0]


def test_pair_entry_point_refusals_launch_nothing():
    """cl_posterior_sample_pair decides its refusals on the host: no GPU is needed to see them return 1."""
    from ctrlora_amd import build, hip
    build.build(verbose=False)
    L = hip.lib()
    p, N = 4096, None                                                    # a non-null stand-in pointer; never dereferenced
    f = L.cl_posterior_sample_pair
    assert "cl_posterior_sample_pair" in hip.EXPORTED
    assert f(N, p, p, N, N, N, 1, 4, 1.0, N) == 1 and f(p, N, p, N, N, N, 1, 4, 1.0, N) == 1 and f(p, p, N, N, N, N, 1, 4, 1.0, N) == 1
    assert f(p, p, p, N, N, N, 0, 4, 1.0, N) == 1 and f(p, p, p, N, N, N, -1, 4, 1.0, N) == 1
    assert f(p, p, p, N, N, N, 1, 0, 1.0, N) == 1 and f(p, p, p, N, N, N, 1, -4, 1.0, N) == 1
    for half in ((p, N, N), (N, p, N), (N, N, p), (p, p, N), (p, N, p), (N, p, p)):
        assert f(p, p, p, *half, 1, 4, 1.0, N) == 1, half
    probe = (__import__("ctypes").c_int * 8)()
    assert L.cl_debug_ew_last_launch(probe) == 0 and probe[0] == 0       # a refused call leaves the launch record empty
