"""The first-stage conformance suite's reference and gate (tests/vae_ref.py), tested without a GPU.

MODEL VALIDATION.  With rounding off, vae_ref equals the repository's own AutoencoderKL torch modules evaluated in fp64 to 1e-12:
every ResnetBlock / AttnBlock / Downsample / Upsample on the input the module itself saw (forward hooks), the folded
conv_out . quant_conv against the unfused 3x3 followed by the 1x1, the zero-padded 32 x 32 post_quant linear against the 1x1
conv, and the whole encoder and decoder -- on the tiny ddconfig (ch = 32, ch_mult = (1, 2, 4, 4), one ResnetBlock per level) at
64 x 32 and 32 x 64, two different images per batch.

GATE VALIDATION.  tests/test_gpu_vae_conformance.py gates a bf16 engine output with the block-conformance rule

    rel-L2(engine, fp64) <= GATE x rel-L2(comparator, fp64),        comparator = vae_ref with Mode(round=True)

on the same bf16-representable inputs.  The study below (5 seeds: other weights, other images; both orientations) measures, per
block form and for the whole encoder / decoder, (a) the floor rel-L2(comparator, fp64) and its seed-to-seed spread max / min,
and (b) for each planted defect of vae_ref.DEFECTS the ratio rel-L2(comparator WITH the defect, fp64) / floor at every place
the defect acts, and keeps the smallest.  The factor 2 stands only if (a) < 2 < (b) everywhere.  Measured (this file prints
the table; `pytest -s`):

    floor rel-L2(comparator, fp64), 5 seeds x 2 sizes          places   floor (min .. max)        largest spread at one place
      encoder (whole)                                             1     9.20e-3 .. 1.35e-2        1.46
      decoder (whole)                                             1     1.24e-2 .. 1.43e-2        1.15
      ResnetBlock                                                12     1.95e-3 .. 4.02e-3        1.21
      ResnetBlock with nin_shortcut                               4     3.00e-3 .. 3.49e-3        1.06
      AttnBlock                                                   2     2.09e-3 .. 2.74e-3        1.23
      Downsample                                                  3     2.27e-3 .. 2.39e-3        1.04
      Upsample                                                    3     2.29e-3 .. 2.40e-3        1.04
      folded conv_out (fp32 out: weight rounding only)            1     1.20e-3 .. 2.28e-3        1.91

    defect error / floor, smallest over seeds, sizes, places    at the block where it acts     through the whole encoder / decoder
      s2a_other_side   Downsample padded (1, 0, 1, 0)                 209                         83
      s2a_symmetric    Downsample as stride 2, pad 1                  209                         83
      attn_scale       softmax scale off by sqrt 2                     32                          6.7
      attn_kv0         K / V of image 0 for every image                59                         10.7
      p_tail           last 32 columns of P not normalised            703                         60
      fold_bias        Q . b_c missing from the folded bias            44                          7.6
      nin_skip         nin_shortcut not added                         220                         83
      up_shift         Upsample source one pixel off                  246                         87
      gn_eps           GroupNorm eps 1e-5 (UNDETECTABLE)                0.99                       0.94

So GATE = 2 is kept: the largest seed-to-seed spread of a floor is 1.91 (the folded conv_out, whose fp32 output carries the weight
rounding alone -- the engine reads the same rounded weights, so its own error sits ON that floor; every block that stores bf16
stays below 1.5), the smallest defect ratio at the block where the defect lives is 32 (attn_scale).  Seen through the WHOLE
encoder / decoder the same defects are diluted to 6.7 at worst -- still above 2, but the margin is five times smaller, which is
why the GPU file gates every launch form on its own and does not rely on the end-to-end figure.
Undetectable by any gate of this kind, and listed instead of dropped: GroupNorm eps 1e-5 against 1e-6 (ratio 0.99: the variance
of a normalised group is of the order of 1, so eps moves the output by ~5e-6 relative, far below one bf16 rounding).
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import vae_ref as VR

GATE = 2.0
SEEDS = (0, 1, 2, 3, 4)
SIZES = ((64, 32), (32, 64))
ROUND = VR.Mode(round=True)
# where each defect acts: (encoder / decoder, block names)
WHERE = {
    "s2a_other_side": ("enc", ("down.0.downsample", "down.1.downsample", "down.2.downsample")),
    "s2a_symmetric": ("enc", ("down.0.downsample", "down.1.downsample", "down.2.downsample")),
    "attn_scale": ("both", ("mid.attn_1",)),
    "attn_kv0": ("both", ("mid.attn_1",)),
    "p_tail": ("both", ("mid.attn_1",)),
    "fold_bias": ("enc", ("conv_out",)),
    "nin_skip": ("enc", ("down.1.block.0", "down.2.block.0")),
    "up_shift": ("dec", ("up.1.upsample", "up.2.upsample", "up.3.upsample")),
    "gn_eps": ("both", ("mid.block_1", "mid.attn_1")),
}


@pytest.fixture(scope="module")
def models():
    return {s: VR.make_model(VR.TINY, s).double() for s in SEEDS}


def _hooked(model, run):
    """{module path: (input, output)} of every ResnetBlock / AttnBlock / Downsample / Upsample during run()."""
    from ldm.models import autoencoder as A
    seen, hooks = {}, []
    for name, mod in model.named_modules():
        if isinstance(mod, (A.ResnetBlock, A.AttnBlock, A._Down, A._Up)):
            hooks.append(mod.register_forward_hook(lambda m, i, o, name=name: seen.__setitem__(name, (i[0].detach(), o.detach()))))
    try:
        with torch.no_grad():
            out = run()
    finally:
        for h in hooks:
            h.remove()
    return seen, out


def _fn_of(name):
    if "attn" in name:
        return VR.attn
    if name.endswith("downsample"):
        return VR.downsample
    if name.endswith("upsample"):
        return VR.upsample
    return VR.resblock


# ------------------------------------------------------------------------------------------------ model validation

@pytest.mark.parametrize("H,W", SIZES)
def test_exact_model_equals_the_torch_modules_block_by_block_and_whole(models, H, W):
    m = models[0]
    sd = VR.state64(m)
    x = VR.image(2, H, W, seed=H).double()
    z = VR.latent(2, H // 8, W // 8, seed=H).double()
    assert not torch.equal(x[0], x[1])
    seen_e, mom = _hooked(m, lambda: m.quant_conv(m.encoder(x)))
    seen_d, img = _hooked(m, lambda: m.decoder(m.post_quant_conv(z)))
    assert len(seen_e) == 4 + 3 + 3 and len(seen_d) == 8 + 3 + 3, (sorted(seen_e), sorted(seen_d))
    kinds = set()
    for seen in (seen_e, seen_d):
        for name, (i, o) in seen.items():
            fn = _fn_of(name)
            kinds.add((fn.__name__, name + ".nin_shortcut.weight" in sd))
            torch.testing.assert_close(fn(sd, name, i), o, rtol=1e-12, atol=1e-12, msg=lambda s, name=name: name + ": " + s)
    assert kinds == {("resblock", False), ("resblock", True), ("attn", False), ("downsample", False), ("upsample", False)}
    taps = {}
    torch.testing.assert_close(VR.encoder(sd, VR.TINY, x, taps=taps), mom, rtol=1e-12, atol=1e-12)
    assert tuple(mom.shape) == (2, 8, H // 8, W // 8) and set(taps) == {n[len("encoder."):] for n in seen_e} | {"conv_out"}
    torch.testing.assert_close(VR.decoder(sd, VR.TINY, z), img, rtol=1e-12, atol=1e-12)
    assert tuple(img.shape) == (2, 3, H, W)
    # rows of one image depend on that image alone: the second image changed, the first image's outputs do not move
    x2 = x.clone()
    x2[1] = -x2[1]
    assert torch.equal(VR.encoder(sd, VR.TINY, x2)[0], VR.encoder(sd, VR.TINY, x)[0])


def test_weight_transformations_equal_what_they_restate(models):
    m = models[1]
    sd = VR.state64(m)
    g = torch.Generator().manual_seed(5)
    hn = torch.randn(2, 128, 8, 4, generator=g).double()
    torch.testing.assert_close(VR.enc_conv_out(sd, hn), VR.enc_conv_out_unfused(sd, hn), rtol=1e-12, atol=1e-12)
    with torch.no_grad():
        torch.testing.assert_close(VR.enc_conv_out(sd, hn), m.quant_conv(m.encoder.conv_out(hn)), rtol=1e-12, atol=1e-12)
    # the bias term Q . b_c is a visible part of it
    assert VR.rel(VR.enc_conv_out(sd, hn, VR.Mode(defect="fold_bias")), VR.enc_conv_out_unfused(sd, hn)) > 1e-2
    z = VR.latent(3, 4, 8).double()
    with torch.no_grad():
        torch.testing.assert_close(VR.post_quant(sd, z), m.post_quant_conv(z), rtol=1e-12, atol=1e-12)
    Wp, bp = VR.post_quant_padded(sd)
    assert tuple(Wp.shape) == (32, 32) and not Wp[4:].any() and not Wp[:, 4:].any() and not bp[4:].any()


def test_rounding_points_round_and_the_fp32_outputs_do_not(models):
    sd = VR.state64(models[2])
    x = VR.image(2, 32, 64, seed=9).double()
    taps = {}
    mom = VR.encoder(sd, VR.TINY, x, ROUND, taps=taps)
    bf = lambda t: torch.equal(t, t.to(torch.bfloat16).double())
    assert all(bf(o) for n, (i, o) in taps.items() if n != "conv_out") and bf(taps["conv_out"][0])
    assert not bf(mom)                                          # the moments stay fp32
    img = VR.decoder(sd, VR.TINY, VR.latent(2, 4, 8).double(), ROUND)
    assert not bf(img)
    f32 = VR.Mode(round=True, dtype=torch.float32)
    assert VR.rel(VR.encoder(sd, VR.TINY, x, f32), VR.encoder(sd, VR.TINY, x)) < 1e-6


# ------------------------------------------------------------------------------------------------ gate validation

def _study(models):
    """floors[name] = [comparator error per (seed, size)], ratios[defect] = [defect error / floor at each place it acts],
    whole[defect] = [the same through the whole encoder / decoder]."""
    floors, ratios, whole = {}, {d: [] for d in WHERE}, {d: [] for d in WHERE}
    rb = lambda t: t.to(torch.bfloat16).double()
    for s in SEEDS:
        sd = VR.state64(models[s])
        for H, W in SIZES:
            x = rb(VR.image(2, H, W, seed=10 * s + H).double())
            z = rb(VR.latent(2, H // 8, W // 8, seed=10 * s + H).double())
            te, td = {}, {}
            ref_e, ref_d = VR.encoder(sd, VR.TINY, x, taps=te), VR.decoder(sd, VR.TINY, z, taps=td)
            fl_e, fl_d = VR.rel(VR.encoder(sd, VR.TINY, x, ROUND), ref_e), VR.rel(VR.decoder(sd, VR.TINY, z, ROUND), ref_d)
            floors.setdefault("encoder", []).append(fl_e)
            floors.setdefault("decoder", []).append(fl_d)
            blocks = {}
            for side, taps in (("enc", te), ("dec", td)):
                for name, (i, o) in taps.items():
                    i = rb(i)
                    if name == "conv_out":
                        fn = lambda sd, p, i, m=VR.EXACT: VR.enc_conv_out(sd, i, m)
                    else:
                        fn = _fn_of(name)
                    p = ("encoder." if side == "enc" else "decoder.") + name
                    ref = fn(sd, p, i)
                    fl = VR.rel(fn(sd, p, i, ROUND), ref)
                    kind = ("conv_out" if name == "conv_out" else fn.__name__ + ("+nin" if p + ".nin_shortcut.weight" in sd else ""))
                    floors.setdefault(f"{kind} {side}.{name}", []).append(fl)
                    blocks[(side, name)] = (fn, p, i, ref, fl)
            for d, (side, names) in WHERE.items():
                md = VR.Mode(round=True, defect=d)
                for sd_ in (("enc", "dec") if side == "both" else (side,)):
                    for name in names:
                        fn, p, i, ref, fl = blocks[(sd_, name)]
                        ratios[d].append(VR.rel(fn(sd, p, i, md), ref) / fl)
                    if sd_ == "enc":
                        whole[d].append(VR.rel(VR.encoder(sd, VR.TINY, x, md), ref_e) / fl_e)
                    else:
                        whole[d].append(VR.rel(VR.decoder(sd, VR.TINY, z, md), ref_d) / fl_d)
    return floors, ratios, whole


def test_gate_factor_separates_the_floor_from_every_planted_defect(models):
    floors, ratios, whole = _study(models)
    print("\nfloor rel-L2(comparator, fp64) over %d seeds x %d sizes:" % (len(SEEDS), len(SIZES)))
    spread, kinds = {}, {}
    for k, v in floors.items():
        spread[k] = max(v) / min(v)                       # one place (the same block of the same network), other seeds
        kinds.setdefault(k.split()[0], []).append((min(v), max(v), spread[k]))
    for k, v in kinds.items():
        print(f"  {k:14s} places {len(v):2d}  floor {min(a for a, _, _ in v):.3e} .. {max(b for _, b, _ in v):.3e}  "
              f"largest spread at one place {max(c for _, _, c in v):.2f}")
    print("defect error / floor: smallest at the block where it acts | smallest through the whole encoder / decoder")
    for d in WHERE:
        print(f"  {d:15s} {min(ratios[d]):10.2f} | {min(whole[d]):8.2f}")
    assert len(SEEDS) >= 5 and all(len(v) >= len(SEEDS) for v in floors.values())
    assert set(VR.DEFECTS) | set(VR.UNDETECTABLE) == set(WHERE)
    assert max(spread.values()) < GATE, spread
    for d in VR.DEFECTS:
        assert min(ratios[d]) > GATE, (d, min(ratios[d]))
    # listed, not dropped: no relative gate at bf16 storage sees it
    for d in VR.UNDETECTABLE:
        assert max(ratios[d]) < GATE, (d, ratios[d])
    assert all(math.isfinite(x) for v in list(ratios.values()) + list(whole.values()) for x in v)
