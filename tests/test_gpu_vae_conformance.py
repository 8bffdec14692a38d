"""The first-stage engine (ctrlora_amd/engine/vae.py), launch form by launch form, against the fp64 model of tests/vae_ref.py
evaluated on the device: every block the engine builds at the shipped widths (128 / 256 / 512 channels) on small grids, the whole
encoder and decoder on the tiny ddconfig, and the routing of AutoencoderKL.encode / decode.

Gates, on every output of every form, in both engine dtypes:

  bf16   rel-L2(engine, fp64) <= GATE x rel-L2(comparator, fp64), comparator = the same model with Mode(round=True): bf16 at the
         tensors the engine stores, on the same inputs.  GATE = 2; tests/test_vae_reference_model.py measures that the floor's
         seed-to-seed spread stays below it (1.91 at most) and every planted defect above it (32 at least at the block where it acts).
  fp32   the parity-mode activation gate of tests/test_gpu_parity.py and the block conformance: 1e-4.
  both   no NaN / Inf in an output; every input bit-identical after the call (x also where it is the residual of a block
         without a shortcut).

The attention block is gated per IMAGE (three different images): a slicing mistake that hands one image the keys of another is a
large error on that image's rows and cannot average out over the batch.  Figures go through _record; test_zz_vae_conformance_summary
records per-form maxima and the wall time of the file.
"""
import json
import time

import pytest
import torch
import torch.nn.functional as F

from tests import vae_ref as VR
from tests.gemm_ref import _tags
from tests.test_gpu_bench_shapes import _need_gpu, _record

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
GATE = 2.0
F32_ACT = 1e-4
_STATS = {}
_T0 = [None]


def _gate(form, dtype, got, ref, cmp, what="out"):
    """Gate one output (the module docstring) and note the figures; returns the failure text or None."""
    if _T0[0] is None:
        _T0[0] = time.time()
    e, f = VR.rel(got, ref), VR.rel(cmp, ref)
    finite = bool(torch.isfinite(got).all())
    s = _STATS.setdefault(form, dict(bf16_ratio=0.0, bf16_rel=0.0, f32_rel=0.0, outputs=0))
    s["outputs"] += 1
    if dtype == BF:
        s["bf16_ratio"], s["bf16_rel"] = max(s["bf16_ratio"], e / f), max(s["bf16_rel"], e)
        ok = finite and f > 0 and e <= GATE * f
    else:
        s["f32_rel"] = max(s["f32_rel"], e)
        ok = finite and e <= F32_ACT
    print(f"[vae conformance] {form} {what} {str(dtype)[6:]}: engine {e:.3e} comparator {f:.3e} finite {finite}")
    _record("vae_conformance/" + form, what=what, dtype=str(dtype), engine=e, comparator=f, finite=finite, passed=ok)
    return None if ok else f"{form} {what}: engine {e:.3e} comparator {f:.3e} finite {finite}"


def _rand(seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return lambda *s, sc=1.0: torch.randn(*s, generator=g, device="cuda") * sc


def _block_sd(kind, cin, cout, seed):
    """fp32 weights of one block under the prefix `blk`, at the scale of a trained network (vae_ref.make_model)."""
    r = _rand(seed)
    sd = {}
    norm = lambda n, c: sd.update({n + ".weight": 1.0 + 0.2 * r(c), n + ".bias": 0.1 * r(c)})
    conv = lambda n, o, i, k: sd.update({n + ".weight": r(o, i, k, k, sc=(i * k * k) ** -0.5), n + ".bias": 0.1 * r(o)})
    if kind == "res":
        norm("blk.norm1", cin); conv("blk.conv1", cout, cin, 3); norm("blk.norm2", cout); conv("blk.conv2", cout, cout, 3)
        if cin != cout:
            conv("blk.nin_shortcut", cout, cin, 1)
    elif kind == "attn":
        norm("blk.norm", cin)
        for n in ("q", "k", "v", "proj_out"):
            conv("blk." + n, cin, cin, 1)
    else:
        conv("blk.conv", cout, cin, 3)
    return sd


def _d(sd):
    return {k: v.double() for k, v in sd.items()}


def _tok(x_nchw, dtype):
    """NCHW values as the engine's token-major rows [B H W, C] in `dtype`."""
    return x_nchw.permute(0, 2, 3, 1).reshape(-1, x_nchw.shape[1]).to(dtype).contiguous()


def _nchw(tok, B, H, W):
    return tok.double().reshape(B, H, W, -1).permute(0, 3, 1, 2)


def _ctx(dtype):
    from ctrlora_amd.engine.blocks import Ctx
    return Ctx(dtype, torch.device("cuda"), False)


def _vb(sd, dtype):
    from ctrlora_amd.engine.vae import _VB
    return _VB(sd, "", dtype, torch.device("cuda"))


def _modes(dtype):
    return VR.EXACT, VR.Mode(round=True, dtype=dtype)


# ------------------------------------------------------------------------------------------------ blocks at the shipped widths

@DTYPES
@pytest.mark.parametrize("cin,cout,B,H,W", [(128, 128, 3, 16, 8), (128, 256, 3, 16, 8), (512, 512, 4, 8, 4)],
                         ids=["128-128", "128-256-nin", "512-512"])
def test_resnet_block(cin, cout, B, H, W, dtype):
    _need_gpu()
    from ctrlora_amd.engine.vae import _VRes
    sd = _block_sd("res", cin, cout, cin + cout)
    blk = _VRes(_vb(sd, dtype), "blk")
    assert (blk.nin is not None) == (cin != cout)               # 128 -> 256: conv2 adds onto the shortcut IN PLACE
    x = _tok(_rand(7)(B, cin, H, W), dtype)
    x0 = x.clone()
    out = blk.fwd(_ctx(dtype), x, B, H, W)
    torch.cuda.synchronize()
    assert torch.equal(x, x0), "the block changed its input"
    exact, rnd = _modes(dtype)
    xin = _nchw(x, B, H, W)
    bad = _gate(f"res{cin}-{cout}", dtype, _nchw(out, B, H, W), VR.resblock(_d(sd), "blk", xin, exact), VR.resblock(_d(sd), "blk", xin, rnd))
    assert not bad, bad


@DTYPES
@pytest.mark.parametrize("H,W", [(8, 4), (8, 12), (16, 16)], ids=["n32", "n96", "n256"])
def test_attention_block_per_image(H, W, dtype):
    _need_gpu()
    from ctrlora_amd.engine.vae import _VAttn
    B, C = 3, 512
    sd = _block_sd("attn", C, C, 40 + H * W)
    # q / k at a scale where the softmax is far from uniform: a wrong key set or a wrong scale moves the output visibly
    for n in ("q", "k"):
        sd[f"blk.{n}.weight"] = sd[f"blk.{n}.weight"] * 3.0
    blk = _VAttn(_vb(sd, dtype), "blk")
    r = _rand(8)
    x4 = torch.stack([r(C, H, W) * (1.0 + 0.5 * b) + 0.3 * b for b in range(B)])        # three different images
    x = _tok(x4, dtype)
    x0 = x.clone()
    out = blk.fwd(_ctx(dtype), x, B, H, W)
    torch.cuda.synchronize()
    assert torch.equal(x, x0), "the block changed its input"
    exact, rnd = _modes(dtype)
    xin = _nchw(x, B, H, W)
    ref, cmp, got = VR.attn(_d(sd), "blk", xin, exact), VR.attn(_d(sd), "blk", xin, rnd), _nchw(out, B, H, W)
    # the reference itself tells the images apart: image 1 with image 0's keys is far outside the gate
    mixed = VR.attn(_d(sd), "blk", xin, VR.Mode(defect="attn_kv0"))
    assert VR.rel(mixed[1], ref[1]) > 10 * GATE * VR.rel(cmp[1], ref[1])
    bad = [_gate(f"attn-n{H * W}", dtype, got[b], ref[b], cmp[b], what=f"image{b}") for b in range(B)]
    assert not any(bad), bad


@DTYPES
@pytest.mark.parametrize("B,H,W", [(3, 16, 24), (2, 32, 16)], ids=["16x24-ragged", "32x16"])
def test_downsample_s2a(B, H, W, dtype):
    _need_gpu()
    from ctrlora_amd import hip
    from ctrlora_amd.engine.blocks import conv3_fwd
    C = 128
    sd = _block_sd("conv", C, C, 60 + H)
    cw = _vb(sd, dtype).conv3("blk.conv")
    x = _tok(VR.image(B, H, W, seed=H, device="cuda")[:, :1].repeat(1, C, 1, 1) + 0.2 * _rand(9)(B, C, H, W), dtype)     # smooth + noise
    x0 = x.clone()
    out = conv3_fwd(_ctx(dtype), cw, x, B, H, W, mode=hip.CONV_S2A)
    torch.cuda.synchronize()
    assert torch.equal(x, x0) and tuple(out.shape) == (B * (H // 2) * (W // 2), C)
    exact, rnd = _modes(dtype)
    xin = _nchw(x, B, H, W)
    ref = VR.downsample(_d(sd), "blk", xin, exact)
    for wrong in ("s2a_other_side", "s2a_symmetric"):           # (the inputs do tell the conventions apart)
        assert VR.rel(VR.downsample(_d(sd), "blk", xin, VR.Mode(defect=wrong)), ref) > 0.1
    bad = _gate(f"down-{H}x{W}", dtype, _nchw(out, B, H // 2, W // 2), ref, VR.downsample(_d(sd), "blk", xin, rnd))
    assert not bad, bad


@DTYPES
@pytest.mark.parametrize("B,phase", [(4, True), (3, False)], ids=["phase", "nine-tap"])
def test_upsample_forms(B, phase, dtype):
    """4 x 8 -> 8 x 16 at 512 channels: B H W = 128 source pixels fill a 128-row tile and take the phase-decomposed product
    (mode 6); B = 3 (96 pixels) takes the nine-tap mode 3.  Which one ran is asserted from the predicate and the launch tags."""
    _need_gpu()
    from ctrlora_amd import hip
    from ctrlora_amd.engine.blocks import _phase_ok, conv3_fwd
    C, H, W = 512, 4, 8
    sd = _block_sd("conv", C, C, 70)
    cw = _vb(sd, dtype).conv3("blk.conv")
    ctx = _ctx(dtype)
    assert _phase_ok(ctx, cw, B, H, W, cw.Ip, cw.Op) == phase
    x = _tok(_rand(10 + B)(B, C, H, W), dtype)
    x0 = x.clone()
    with _tags():
        out = conv3_fwd(ctx, cw, x, B, H, W, mode=hip.CONV_UP2)
        torch.cuda.synchronize()
        modes = [t["mode"] for t in hip.gemm_tags()]
    assert modes == [hip.CONV_UP2P if phase else hip.CONV_UP2], modes
    assert torch.equal(x, x0)
    exact, rnd = _modes(dtype)
    xin = _nchw(x, B, H, W)
    ref = VR.upsample(_d(sd), "blk", xin, exact)
    assert VR.rel(VR.upsample(_d(sd), "blk", xin, VR.Mode(defect="up_shift")), ref) > 0.1
    bad = _gate("up-phase" if phase else "up-nine-tap", dtype, _nchw(out, B, 2 * H, 2 * W), ref, VR.upsample(_d(sd), "blk", xin, rnd))
    assert not bad, bad


@DTYPES
def test_conv_in_from_an_nchw_image(dtype):
    """conv_in 3 -> 128: the fp32 NCHW image through nchw_to_tok into 32 token columns (29 of them zero padding), then the 3x3."""
    _need_gpu()
    from ctrlora_amd import hip
    from ctrlora_amd.engine.blocks import conv3_fwd
    from ctrlora_amd.engine.packing import rup
    B, H, W = 3, 16, 8
    sd = _block_sd("conv", 3, 128, 80)
    cw = _vb(sd, dtype).conv3("blk.conv")
    assert (cw.Ip, cw.Op) == (32, 128)
    img = VR.image(B, H, W, seed=3, device="cuda")
    img0 = img.clone()
    tok = torch.full((B * H * W, rup(3, 32)), float("nan"), dtype=dtype, device="cuda")
    hip.nchw_to_tok(img, tok)
    out = conv3_fwd(_ctx(dtype), cw, tok, B, H, W)
    torch.cuda.synchronize()
    assert torch.equal(img, img0) and not tok[:, 3:].any() and torch.equal(tok[:, :3], _tok(img, dtype))
    exact, rnd = _modes(dtype)
    f = lambda m: VR.S(m, VR.conv3(_d(sd), "blk.conv", VR.S(m, img.double()), m, padding=1))
    bad = _gate("conv_in", dtype, _nchw(out, B, H, W), f(exact), f(rnd))
    assert not bad, bad


@DTYPES
def test_decoder_conv_out_to_an_fp32_image(dtype):
    """conv_out 128 -> 3: a ragged output width (3 of 32 padded columns are real) stored as fp32, then tok_to_nchw."""
    _need_gpu()
    from ctrlora_amd import hip
    from ctrlora_amd.engine.blocks import conv3_fwd
    B, H, W = 3, 16, 8
    sd = _block_sd("conv", 128, 3, 81)
    cw = _vb(sd, dtype).conv3("blk.conv")
    assert (cw.Ip, cw.Op) == (128, 32)
    x = _tok(_rand(12)(B, 128, H, W), dtype)
    x0 = x.clone()
    tok = conv3_fwd(_ctx(dtype), cw, x, B, H, W, out_f32=True)
    out = torch.full((B, 3, H, W), float("nan"), dtype=F32, device="cuda")
    hip.tok_to_nchw(tok, out)
    torch.cuda.synchronize()
    assert torch.equal(x, x0) and tok.dtype == F32
    exact, rnd = _modes(dtype)
    xin = _nchw(x, B, H, W)
    f = lambda m: VR.conv3(_d(sd), "blk.conv", xin, m, padding=1)        # fp32 out: not rounded
    bad = _gate("dec_conv_out", dtype, out, f(exact), f(rnd))
    assert not bad, bad


@pytest.fixture(scope="module")
def tiny():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    m = VR.make_model(VR.TINY, 11).cuda()
    return m, VR.state64(m, "cuda"), {k: v.detach() for k, v in m.state_dict().items()}


@DTYPES
def test_encoder_folded_conv_out_against_the_unfused_pair(tiny, dtype):
    """The encoder's own fold (VAEEncoderE.__init__) on a norm_out-like input, against the UNFUSED 3x3 followed by the 1x1 in fp64."""
    _need_gpu()
    from ctrlora_amd.engine.blocks import conv3_fwd
    from ctrlora_amd.engine.vae import VAEEncoderE
    _, sd64, sd = tiny
    enc = VAEEncoderE(sd, VR.TINY, dtype, "cuda")
    B, H, W, C = 2, 8, 4, 128
    hn = _tok(_rand(13)(B, C, H, W), dtype)
    hn0 = hn.clone()
    tok = conv3_fwd(_ctx(dtype), enc.conv_out, hn, B, H, W, out_f32=True)
    torch.cuda.synchronize()
    assert torch.equal(hn, hn0) and enc.out_ch == 8
    xin = _nchw(hn, B, H, W)
    ref = VR.enc_conv_out_unfused(sd64, xin)
    assert VR.rel(VR.enc_conv_out(sd64, xin, VR.Mode(defect="fold_bias")), ref) > 1e-2
    bad = _gate("enc_conv_out_folded", dtype, _nchw(tok[:, :8], B, H, W), ref, VR.enc_conv_out(sd64, xin, VR.Mode(round=True, dtype=dtype)))
    assert not bad, bad
    assert not tok[:, 8:].any(), "the padded output columns of the folded conv carry zero weights and zero bias"


@DTYPES
def test_post_quant_padded_linear(tiny, dtype):
    _need_gpu()
    from ctrlora_amd import hip
    from ctrlora_amd.engine.blocks import linear_fwd
    from ctrlora_amd.engine.vae import VAEDecoderE
    _, sd64, sd = tiny
    dec = VAEDecoderE(sd, VR.TINY, dtype, "cuda")
    B, H, W = 3, 4, 8
    z = VR.latent(B, H, W, seed=5, device="cuda")
    z0 = z.clone()
    tok = torch.full((B * H * W, 32), float("nan"), dtype=dtype, device="cuda")
    hip.nchw_to_tok(z, tok)
    zq, _ = linear_fwd(_ctx(dtype), dec.post_quant, tok)
    torch.cuda.synchronize()
    assert torch.equal(z, z0) and tuple(zq.shape) == (B * H * W, 32) and not zq[:, 4:].any()
    exact, rnd = _modes(dtype)
    ref = F.conv2d(z.double(), sd64["post_quant_conv.weight"], sd64["post_quant_conv.bias"])      # what the padded linear restates
    torch.testing.assert_close(VR.post_quant(sd64, z.double(), exact), ref, rtol=1e-12, atol=1e-12)
    bad = _gate("post_quant", dtype, _nchw(zq[:, :4], B, H, W), ref, VR.post_quant(sd64, z.double(), rnd))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ whole encoder / decoder (tiny)

@DTYPES
@pytest.mark.parametrize("H,W", [(64, 32), (32, 64), (64, 96)], ids=["64x32", "32x64", "64x96"])
def test_whole_encoder(tiny, H, W, dtype):
    _need_gpu()
    from ctrlora_amd.engine.vae import VAEEncoderE
    _, sd64, sd = tiny
    x = VR.image(2, H, W, seed=H + W, device="cuda")
    assert not torch.equal(x[0], x[1])
    x0 = x.clone()
    got = VAEEncoderE(sd, VR.TINY, dtype, "cuda")(x)
    torch.cuda.synchronize()
    assert torch.equal(x, x0) and tuple(got.shape) == (2, 8, H // 8, W // 8) and got.dtype == F32
    exact, rnd = _modes(dtype)
    bad = _gate("encoder", dtype, got, VR.encoder(sd64, VR.TINY, x.double(), exact), VR.encoder(sd64, VR.TINY, x.double(), rnd), what=f"{H}x{W}")
    assert not bad, bad


@DTYPES
@pytest.mark.parametrize("h,w", [(8, 4), (4, 8), (8, 12)], ids=["8x4", "4x8", "8x12"])
def test_whole_decoder(tiny, h, w, dtype):
    _need_gpu()
    from ctrlora_amd.engine.vae import VAEDecoderE
    _, sd64, sd = tiny
    z = VR.latent(2, h, w, seed=h + w, device="cuda")
    z0 = z.clone()
    got = VAEDecoderE(sd, VR.TINY, dtype, "cuda")(z)
    torch.cuda.synchronize()
    assert torch.equal(z, z0) and tuple(got.shape) == (2, 3, 8 * h, 8 * w) and got.dtype == F32
    exact, rnd = _modes(dtype)
    bad = _gate("decoder", dtype, got, VR.decoder(sd64, VR.TINY, z.double(), exact), VR.decoder(sd64, VR.TINY, z.double(), rnd), what=f"{h}x{w}")
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ routing

def test_routing_of_shapes_the_engine_does_not_take(tiny, monkeypatch):
    """Shapes the engine cannot take go to the torch modules instead of raising: exactly what use_engine = False returns, and no
    engine is built.  An accepted shape builds it -- unless the attention row limit says otherwise."""
    _need_gpu()
    m = tiny[0]
    m.engine_dtype = F32
    m.invalidate_engine()
    x_bad, z_bad = VR.image(1, 40, 24, seed=1, device="cuda"), VR.latent(1, 5, 3, seed=1, device="cuda")
    # (accepted: image sides multiples of 8 with H W % 2048 == 0; latent sides multiples of 8 -- _on_engine asks that of the
    # latent as well, so an 8 x 4 latent, which the decoder engine itself takes, is routed to the torch modules too)
    x_ok, z_ok = VR.image(1, 64, 32, seed=2, device="cuda"), VR.latent(1, 8, 8, seed=2, device="cuda")
    assert (40 * 24) % 2048 and (5 * 3) % 32
    with torch.no_grad():
        m.use_engine = False
        ref = [m.encode(x_bad).parameters, m.decode(z_bad), m.encode(x_ok).parameters, m.decode(z_ok)]
        m.use_engine = True
        got = [m.encode(x_bad).parameters, m.decode(z_bad)]
        assert "_enc" not in m.__dict__ and "_dec" not in m.__dict__
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
        # an accepted shape under a row limit it exceeds (8 x 4 = 32 and 8 x 8 = 64 latent positions > 16): the torch modules again
        monkeypatch.setattr(type(m), "ENGINE_MAX_ATTN_TOKENS", 16)
        got = [m.encode(x_ok).parameters, m.decode(z_ok)]
        assert "_enc" not in m.__dict__ and "_dec" not in m.__dict__
        assert torch.equal(got[0], ref[2]) and torch.equal(got[1], ref[3])
        monkeypatch.undo()
        got = [m.encode(x_ok).parameters, m.decode(z_ok)]
        assert "_enc" in m.__dict__ and "_dec" in m.__dict__          # the engine ran
        assert got[0].shape == ref[2].shape and got[1].shape == ref[3].shape          # (its numbers: the whole-model tests above)
    m.invalidate_engine()


def test_zz_vae_conformance_summary():
    """Per-form maxima and the wall time of this file, for DESIGN.md."""
    _need_gpu()
    wall = None if _T0[0] is None else time.time() - _T0[0]
    print("vae conformance:", json.dumps(_STATS), "wall_s:", wall)
    _record("vae_conformance/summary", forms=_STATS, wall_s=wall, gate=GATE, f32_gate=F32_ACT)
    for form, s in _STATS.items():
        assert s["bf16_ratio"] <= GATE and s["f32_rel"] <= F32_ACT, (form, s)
