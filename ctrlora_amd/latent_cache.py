"""On-disk cache of first-stage posteriors for fine-tuning on a fixed set of image pairs.

`datasets.custom_dataset.CustomDataset` has no crop, flip or resize: the frozen VAE encoder computes the same posterior for
the same image in every epoch.  The reference keeps the POSTERIOR and draws a fresh sample per step
(LatentDiffusion.get_first_stage_encoding, DiagonalGaussianDistribution.sample); a cache of posteriors reproduces that
distribution draw for draw, a cache of latents would not.

    DIR/target_moments.npy   fp32 [N, 2C, h, w]   (posterior.mean | posterior.std) of item["jpg"]
    DIR/hint_moments.npy     fp32 [N, 2C, h, w]   the same of item["hint"]
    DIR/meta.json            format version, N, latent shape, the records of prompt.json in index order, the engine dtype the
                             encoder ran in, a sha256 fingerprint of the first_stage_model state dict

`std` is stored, not `logvar`: a draw is then scale_factor * (mean + std * e), multiplications and additions only, which the
pair kernel (cl_posterior_sample_pair) evaluates with the roundings of the live path.  The moments are unscaled.

A cache is written under temporary names.  Once all of it is encoded, an older cache's meta.json is removed, the arrays are renamed
into place and the new meta.json last: a directory without meta.json does not load, and a build that fails leaves an older cache
as it was.
"""
from __future__ import annotations

import hashlib
import json
import os

import numpy as np
import torch

FORMAT_VERSION = 1
TARGET, HINT, META = "target_moments.npy", "hint_moments.npy", "meta.json"


class LatentCacheError(ValueError):
    pass


def dtype_name(dtype) -> str:
    return "fp32" if dtype == torch.float32 else "bf16"


def state_fingerprint(module) -> str:
    """sha256 over the names, dtypes, shapes and bytes of a module's state dict, in key order."""
    h = hashlib.sha256()
    sd = module.state_dict()
    for k in sorted(sd):
        v = sd[k].detach().cpu().contiguous()
        h.update(k.encode() + b"\0" + str(v.dtype).encode() + b"\0" + str(tuple(v.shape)).encode() + b"\0")
        h.update(v.reshape(-1).view(torch.uint8).numpy().tobytes() if v.numel() else b"")
    return h.hexdigest()


def _nchw(a, device):
    """The layout handling of LatentDiffusion.get_input / ControlLDM.get_input: [b, H, W, 3] items -> NCHW fp32 on the device."""
    x = torch.from_numpy(np.stack(a))
    return x.to(device).permute(0, 3, 1, 2).to(memory_format=torch.contiguous_format).float()


def _moments(post) -> np.ndarray:
    return torch.cat([post.mean, post.std], 1).float().cpu().numpy()


def build_cache(dataset, encode, out_dir, bs=16, device="cpu", engine_dtype="fp32", fingerprint=""):
    """Walk `dataset` (a CustomDataset with drop_rate 0) in index order and store the posterior `encode` returns for every
    target and condition image.  `encode(x)` takes an NCHW fp32 batch and returns a DiagonalGaussianDistribution
    (LatentDiffusion.encode_first_stage).  Returns the meta dict."""
    N = len(dataset)
    if N < 1:
        raise LatentCacheError("the dataset is empty: nothing to cache")
    os.makedirs(out_dir, exist_ok=True)
    final = {k: os.path.join(out_dir, k) for k in (TARGET, HINT, META)}
    tmp = {k: v + f".tmp{os.getpid()}" for k, v in final.items()}
    for f in os.listdir(out_dir):              # what a killed build left behind
        if any(f.startswith(k + ".tmp") for k in final):
            os.remove(os.path.join(out_dir, f))
    maps, size, shape = None, None, None
    try:
        for lo in range(0, N, bs):
            items = [dataset[i] for i in range(lo, min(lo + bs, N))]
            for i, it in enumerate(items):
                got = (tuple(it["jpg"].shape), tuple(it["hint"].shape))
                size = size or got
                if got != size or got[0] != got[1]:
                    rec = dataset.data[lo + i]
                    raise LatentCacheError(f"images of differing sizes cannot be cached (nor batched by the loader): record {lo + i} "
                                           f"({rec['target']}, {rec['source']}) is {got[0][:2]} / {got[1][:2]}, the first is {size[0][:2]}")
            mom = [_moments(encode(_nchw([it[k] for it in items], device))) for k in ("jpg", "hint")]
            if maps is None:
                shape = tuple(mom[0].shape[1:])
                if shape[0] % 2 or mom[1].shape[1:] != shape:
                    raise LatentCacheError(f"the encoder returned moments of shape {shape} / {tuple(mom[1].shape[1:])}")
                maps = [np.lib.format.open_memmap(tmp[k], mode="w+", dtype=np.float32, shape=(N,) + shape) for k in (TARGET, HINT)]
            for m, a in zip(maps, mom):
                m[lo:lo + len(items)] = a
        for m in maps:
            m.flush()
        del maps
        meta = dict(format_version=FORMAT_VERSION, N=N, latent_shape=[shape[0] // 2, shape[1], shape[2]],
                    records=[dict(r) for r in dataset.data], engine_dtype=engine_dtype, first_stage_sha256=fingerprint)
        with open(tmp[META], "w") as f:
            json.dump(meta, f)
        # everything is encoded and validated: only now does an older cache stop loading (its meta.json goes first), and the new
        # meta.json comes last -- a directory without it is not a cache
        if os.path.exists(final[META]):
            os.remove(final[META])
        for k in (TARGET, HINT, META):
            os.replace(tmp[k], final[k])
        return meta
    finally:
        maps = None
        for p in tmp.values():
            if os.path.exists(p):
                os.remove(p)


def load_meta(cache_dir):
    path = os.path.join(cache_dir, META)
    if not os.path.isfile(path):
        raise LatentCacheError(f"{cache_dir} holds no latent cache ({META} not found): build one with scripts/tool_cache_latents.py")
    with open(path) as f:
        meta = json.load(f)
    if meta.get("format_version") != FORMAT_VERSION:
        raise LatentCacheError(f"{path}: format version {meta.get('format_version')}, this code reads {FORMAT_VERSION}")
    return meta


def open_cache(cache_dir):
    """(meta, target moments, hint moments) with the arrays memory-mapped read-only and checked against meta."""
    meta = load_meta(cache_dir)
    want = (meta["N"], 2 * meta["latent_shape"][0], meta["latent_shape"][1], meta["latent_shape"][2])
    arrs = []
    for k in (TARGET, HINT):
        a = np.load(os.path.join(cache_dir, k), mmap_mode="r")
        if a.dtype != np.float32 or tuple(a.shape) != want:
            raise LatentCacheError(f"{os.path.join(cache_dir, k)} is {a.dtype} {tuple(a.shape)}, {META} says float32 {want}")
        arrs.append(a)
    return meta, arrs[0], arrs[1]


def check_records(meta, records, where="prompt.json"):
    """The cache was built over exactly these records, in this order."""
    if meta["N"] != len(records):
        raise LatentCacheError(f"the latent cache holds {meta['N']} items, {where} lists {len(records)}")
    for i, (a, b) in enumerate(zip(meta["records"], records)):
        if a != b:
            raise LatentCacheError(f"the latent cache differs from {where} at record {i}: cached {a}, listed {b}")


def check_model(meta, model, engine_dtype=None):
    """The cache was encoded by this model's first stage (and, when given, in this engine dtype)."""
    got = state_fingerprint(model.first_stage_model)
    if got != meta["first_stage_sha256"]:
        raise LatentCacheError("the latent cache was built with another first_stage_model: state-dict sha256 "
                               f"{meta['first_stage_sha256'][:16]}... in the cache, {got[:16]}... in the model")
    if engine_dtype is not None and meta["engine_dtype"] != dtype_name(engine_dtype):
        raise LatentCacheError(f"the latent cache was encoded in {meta['engine_dtype']}, training runs the engine in "
                               f"{dtype_name(engine_dtype)}: rebuild it with the matching --precision")
