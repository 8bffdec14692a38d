"""The cl_gemm conformance suite's reference and checks (tests/gemm_ref.py), tested without a GPU.

  * gemm_ref64 against plain torch on hand-written cases of each epilogue feature of cl_gemm_params;
  * the contract emulated on the CPU (operands in bf16 / fp32, fp32 matmul, split-K partial sums in fp32, fp32 epilogue, ONE
    rounding of the output) passes checks 1 - 3 -- the element-wise bound is not tighter than arithmetic the contract allows;
  * negative controls: each defect is flagged by the check it is named for, so the bound is not looser than the defects it is
    there to catch (the last 32 k of ONE row, ONE element 4 bf16 ulps off, one guard row / pad column written, a row left NaN).
"""
import pytest
import torch

from tests import gemm_ref as G

F = torch.nn.functional
BF, F32 = torch.bfloat16, torch.float32


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ops(g, M, N, K1, K2=0, dtype=BF):
    mk = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(dtype)
    o = dict(a1=mk(M, K1), w1=mk(N, K1, sc=K1 ** -0.5), bias=torch.randn(N, generator=g) * 0.1)
    if K2:
        o.update(a2=mk(M, K2), w2=mk(N, K2, sc=K2 ** -0.5))
    return o


def emulate(c, splits=1):
    """The contract as the kernels may legitimately evaluate it: fp32 products summed per K split, the partial sums added in
    fp32, the epilogue in fp32, one rounding to the output type.  Returns a Guarded output."""
    f = lambda t: None if t is None else t.float()
    M = c["M"]
    if c["mode"] != G.LINEAR or c["a1_group_n"] or c["a2_group_n"] or c["act"] == G.ACT_GEGLU:
        acc = None          # (the fp32 evaluation of the whole expression: no split)
        out = G.gemm_ref64(c, dtype=F32)
    else:
        a = f(c["a1"]) if c["a2"] is None else torch.cat([f(c["a1"]), f(c["a2"])], 1)
        w = f(c["w1"]) if c["a2"] is None else torch.cat([f(c["w1"]), f(c["w2"])], 1)
        K = a.shape[1]
        edges = [K * i // splits // 32 * 32 for i in range(splits)] + [K]
        acc = torch.zeros(M, c["N"])
        for i in range(splits):
            acc = acc + a[:, edges[i]:edges[i + 1]] @ w[:, edges[i]:edges[i + 1]].t()
        if c["bias"] is not None:
            acc = acc + c["bias"]
        if c["rowbias"] is not None:
            acc = acc + f(c["rowbias"])[torch.arange(M) // c["rows_per_batch"]]
        if c["act"] == G.ACT_SILU:
            acc = acc * torch.sigmoid(acc)
        if c["alpha"] != 1.0:
            n = c["alpha_n"] or c["N"]
            acc = torch.cat([acc[:, :n] * c["alpha"], acc[:, n:]], 1)
        if c["residual"] is not None:
            acc = acc + c["beta"] * f(c["residual"])
        if c["atomic"]:
            acc = acc + c["c0"]
        out = acc
    guard = G.Guarded(M, c["out_cols"], c["out_dtype"], "cpu")
    guard.view.copy_(out.to(c["out_dtype"]))
    return guard


# ------------------------------------------------------------------------------------------------ gemm_ref64 vs plain torch

def test_reference_linear_epilogues_vs_plain_torch():
    g = _gen(1)
    M, N, K1, K2 = 154, 160, 64, 32
    o = _ops(g, M, N, K1, K2, dtype=F32)
    a1, w1, a2, w2, bias = (o[k].double() for k in ("a1", "w1", "a2", "w2", "bias"))
    base = a1 @ w1.t() + a2 @ w2.t() + bias
    rb = torch.randn(2, N, generator=g)
    res = torch.randn(M, N, generator=g)
    rows = torch.arange(M) // 77
    eq = lambda c, want: torch.testing.assert_close(G.gemm_ref64(c), want, rtol=1e-12, atol=1e-12)
    eq(G.make_case(**o), base)
    eq(G.make_case(**o, rowbias=rb, rows_per_batch=77), base + rb.double()[rows])
    eq(G.make_case(**o, residual=res, alpha=0.7, beta=-0.5), base * 0.7 - 0.5 * res.double())
    eq(G.make_case(**o, alpha=0.25, alpha_n=48), torch.cat([base[:, :48] * 0.25, base[:, 48:]], 1))
    eq(G.make_case(**o, act=G.ACT_SILU, alpha=2.0), F.silu(base) * 2.0)
    eq(G.make_case(**o, out_f32=True), base)
    eq(G.make_case(**o, atomic=True, splitk=3, c0=1.0), base + 1.0)
    assert G.make_case(**o, out_f32=True)["out_dtype"] == F32 and G.make_case(**_ops(g, 8, 8, 32))["out_dtype"] == BF
    # rows [lo, hi) are rows of the whole
    c = G.make_case(**o, rowbias=rb, rows_per_batch=77, residual=res, beta=1.0)
    torch.testing.assert_close(G.gemm_ref64(c, 70, 100), G.gemm_ref64(c)[70:100], rtol=0, atol=0)
    # mag: the same expression on absolute values
    want = (a1.abs() @ w1.abs().t() + a2.abs() @ w2.abs().t() + bias.abs() + rb.double().abs()[rows]) * 0.7 + 0.5 * res.double().abs()
    eq_abs = G.gemm_ref64(G.make_case(**o, rowbias=rb, rows_per_batch=77, residual=res, alpha=-0.7, beta=-0.5), absolute=True)
    torch.testing.assert_close(eq_abs, want, rtol=1e-12, atol=1e-12)


def test_reference_geglu_is_the_permuted_row_layout_of_geglu_pack():
    """ACT_GEGLU on the rows packing.LinearW.geglu_pack permutes == value * gelu(gate) on the natural [value | gate] rows
    (ldm/modules/attention.py:49-56)."""
    from ctrlora_amd.engine.packing import LinearW
    g = _gen(2)
    M, K, N = 37, 64, 640
    W, b, x = torch.randn(N, K, generator=g) / 8, torch.randn(N, generator=g), torch.randn(M, K, generator=g)
    Wg, bg, _ = LinearW(W, b, F32, "cpu", False).geglu_pack()
    val, gate = (x.double() @ W.double().t() + b.double()).chunk(2, dim=1)
    c = G.make_case(x, Wg, bias=bg, act=G.ACT_GEGLU)
    assert c["out_cols"] == N // 2
    torch.testing.assert_close(G.gemm_ref64(c), val * F.gelu(gate), rtol=1e-12, atol=1e-12)


def test_reference_grouped_segments_vs_plain_torch():
    g = _gen(3)
    M, K, N, r, Gn = 50, 64, 64, 32, 3
    x, W, t, Bm = (torch.randn(*s, generator=g) for s in ((M, K), (Gn * N, K), (M, Gn * r), (Gn * N, r)))
    want = torch.cat([x.double() @ W.double()[i * N:(i + 1) * N].t() + t.double()[:, i * r:(i + 1) * r] @ Bm.double()[i * N:(i + 1) * N].t()
                      for i in range(Gn)], 1)
    torch.testing.assert_close(G.gemm_ref64(G.make_case(x, W, a2=t, w2=Bm, a2_group_n=N)), want, rtol=1e-12, atol=1e-12)
    dy, Bt = torch.randn(M, Gn * N, generator=g), torch.randn(Gn * r, N, generator=g)
    want = torch.cat([dy.double()[:, i * N:(i + 1) * N] @ Bt.double()[i * r:(i + 1) * r].t() for i in range(Gn)], 1)
    torch.testing.assert_close(G.gemm_ref64(G.make_case(dy, Bt, a1_group_n=r)), want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("B,H,W", [(3, 5, 7), (2, 9, 6)])
def test_reference_conv_modes_vs_plain_torch(B, H, W):
    g = _gen(B + H)
    Cin, Cout = 32, 40
    w = torch.randn(Cout, Cin, 3, 3, generator=g).double()
    x = torch.randn(B, Cin, H, W, generator=g).double()
    b = torch.randn(Cout, generator=g)
    pix = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])
    wp = w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin)                    # [N][ky][kx][c]
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    cases = [(G.CONV_S1, (B, H, W, H, W), F.conv2d(x, w, b.double(), padding=1)),
             (G.CONV_S2, (B, H, W, Ho, Wo), F.conv2d(x, w, b.double(), stride=2, padding=1)),
             (G.CONV_UP2, (B, H, W, 2 * H, 2 * W), F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, b.double(), padding=1)),
             # the data gradient of a stride-2 conv whose weight is the tap-flipped, transposed w
             (G.CONV_T2, (B, H, W, 2 * H, 2 * W),
              F.conv_transpose2d(x, w.flip(2, 3).permute(1, 0, 2, 3), b.double(), stride=2, padding=1, output_padding=1))]
    for mode, conv, want in cases:
        c = G.make_case(pix(x), wp, bias=b, mode=mode, conv=conv)
        assert c["M"] == B * conv[3] * conv[4] and c["K1"] == Cin
        torch.testing.assert_close(G.gemm_ref64(c), pix(want), rtol=1e-11, atol=1e-11)
        per = conv[3] * conv[4]
        torch.testing.assert_close(G.gemm_ref64(c, per, 2 * per), pix(want)[per:2 * per], rtol=1e-11, atol=1e-11)
        assert G.k_total(c) == 9 * Cin + 1


@pytest.mark.parametrize("B,H,W", [(3, 6, 10), (2, 9, 7)], ids=["even", "odd"])
def test_reference_conv_s2a_is_the_bottom_right_padded_stride_2_conv(B, H, W):
    """Mode 5 (AutoencoderKL's Downsample) == conv2d(pad(x, (0, 1, 0, 1)), stride 2) in fp64, the magnitude path included -- and
    NOT the two conventions it could silently coincide with: mode 2 (pad 1 on every side) and the pad on the other side
    (1, 0, 1, 0).  Both put every output one input pixel off, so they differ from mode 5 by the size of the output itself."""
    g = _gen(50 + H)
    Cin, Cout = 32, 40
    w = torch.randn(Cout, Cin, 3, 3, generator=g).double()
    x = torch.randn(B, Cin, H, W, generator=g).double()
    b = torch.randn(Cout, generator=g)
    pix = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])
    wp = w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin)
    Ho, Wo = H // 2, W // 2
    want = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b.double(), stride=2)
    assert tuple(want.shape[2:]) == (Ho, Wo)
    c = G.make_case(pix(x), wp, bias=b, mode=G.CONV_S2A, conv=(B, H, W, Ho, Wo))
    assert G.CONV_S2A == 5 and c["M"] == B * Ho * Wo and c["K1"] == Cin and G.k_total(c) == 9 * Cin + 1
    got = G.gemm_ref64(c)
    torch.testing.assert_close(got, pix(want), rtol=1e-11, atol=1e-11)
    per = Ho * Wo
    torch.testing.assert_close(G.gemm_ref64(c, per, 2 * per), pix(want)[per:2 * per], rtol=1e-11, atol=1e-11)
    mag = F.conv2d(F.pad(x.abs(), (0, 1, 0, 1)), w.abs(), b.double().abs(), stride=2)
    torch.testing.assert_close(G.gemm_ref64(c, absolute=True), pix(mag), rtol=1e-11, atol=1e-11)
    # the wrong conventions on the same inputs, cropped to the same grid
    sym = F.conv2d(x, w, b.double(), stride=2, padding=1)[:, :, :Ho, :Wo]
    other = F.conv2d(F.pad(x, (1, 0, 1, 0)), w, b.double(), stride=2)[:, :, :Ho, :Wo]
    for name, wrong in (("pad 1", sym), ("pad (1, 0, 1, 0)", other)):
        assert G._rel(pix(wrong), got) > 0.5, name
    # ... and the element-wise check flags such a result on nearly every element
    res = G.run_checks(dict(c, out_dtype=torch.float32), pix(sym).contiguous())
    assert "elementwise" in G.failures(res) and res["violations"] > 0.9 * c["M"] * Cout, res


def test_row_chunks_tile_every_row_once():
    g = _gen(4)
    c = G.make_case(**_ops(g, 1000, 64, 32))
    for budget in (1 << 12, 1 << 14, 1 << 25):
        ch = G.row_chunks(c, budget)
        assert ch[0][0] == 0 and ch[-1][1] == 1000 and all(a[1] == b[0] for a, b in zip(ch, ch[1:]))
    x = torch.randn(6 * 5 * 7, 32, generator=g)
    c = G.make_case(x, torch.randn(8, 288, generator=g), mode=G.CONV_S1, conv=(6, 5, 7, 5, 7))
    ch = G.row_chunks(c, 1 << 8)
    assert ch[0][0] == 0 and ch[-1][1] == 210 and all(a[1] == b[0] and a[1] % 35 == 0 for a, b in zip(ch, ch[1:]))


# ------------------------------------------------------------------------------------------------ the emulated contract passes

@pytest.mark.parametrize("M,N,K1,K2,splits", [(512, 1280, 1280, 0, 1), (2048, 320, 320, 128, 1), (512, 320, 11520, 0, 8),
                                              (1000, 640, 2560, 512, 3), (4096, 64, 128, 0, 1)])
def test_emulated_contract_passes_checks(M, N, K1, K2, splits):
    c = G.make_case(**_ops(_gen(M + N), M, N, K1, K2))
    guard = emulate(c, splits)
    res = G.run_checks(c, guard.view, guard, budget=1 << 22)            # (several chunks: the accumulation over chunks runs too)
    assert G.failures(res) == [], res
    assert 0.05 < res["err_over_bound"] < 1.0, res                      # the bound is of the size of the error, and above it


def test_emulated_contract_passes_checks_across_the_epilogues():
    g = _gen(9)
    M, N = 231, 320
    o = _ops(g, M, N, 96, 32)
    rb = (torch.randn(3, N, generator=g)).to(BF)
    res = torch.randn(M, N, generator=g).to(BF)
    o32 = _ops(g, M, N, 48, 16, dtype=F32)
    x = torch.randn(3 * 5 * 7, 32, generator=g).to(BF)
    wc = (torch.randn(72, 288, generator=g) / 17).to(BF)
    cases = [G.make_case(**o, rowbias=rb, rows_per_batch=77), G.make_case(**o, residual=res, alpha=0.7, beta=-0.5),
             G.make_case(**o, alpha=0.125, alpha_n=160), G.make_case(**o, act=G.ACT_SILU), G.make_case(**o, act=G.ACT_GEGLU),
             G.make_case(**o, out_f32=True), G.make_case(**o, atomic=True, splitk=3, c0=1.0), G.make_case(**o32),
             G.make_case(**o32, act=G.ACT_SILU, residual=res.float(), beta=1.0),
             G.make_case(x, wc, bias=torch.randn(72, generator=g), mode=G.CONV_S1, conv=(3, 5, 7, 5, 7)),
             G.make_case(x, wc, mode=G.CONV_T2, conv=(3, 5, 7, 10, 14))]
    for i, c in enumerate(cases):
        guard = emulate(c, 3 if c["atomic"] else 1)
        r = G.run_checks(c, guard.view, guard)
        assert G.failures(r) == [], (i, r)


# ------------------------------------------------------------------------------------------------ negative controls

def _clean(M=1000, N=640, K1=1280, K2=0, dtype=BF):
    c = G.make_case(**_ops(_gen(5), M, N, K1, K2, dtype=dtype))
    return c, emulate(c)


@pytest.mark.parametrize("K1,K2", [(64, 0), (320, 128), (1280, 0)])
def test_last_32_k_of_one_row_dropped_is_flagged_by_the_elementwise_check(K1, K2):
    """A tile-tail bug: one output row misses the last 32 k.  Check 2 flags nearly every element of that row; the whole-matrix
    rel-L2 moves by sqrt(32 / (K M)) at most, 5.5e-3 for one row of the production M = 32768 even if the row were lost entirely."""
    c, guard = _clean(K1=K1, K2=K2)
    row = 777
    short = dict(c)
    if K2:
        short["a2"] = c["a2"].clone()
        short["a2"][row, -32:] = 0
    else:
        short["a1"] = c["a1"].clone()
        short["a1"][row, -32:] = 0
    guard.view[row] = emulate(short).view[row]
    res = G.run_checks(c, guard.view, guard)
    assert "elementwise" in G.failures(res) and "canary" not in G.failures(res), res
    assert res["first_violation"]["row"] == row and res["first_violation"]["rows_hit"] == 1
    assert res["violations"] > 0.9 * c["N"], res                        # nearly every element of that row
    assert res["rel"] < 2.5e-2                                          # what this moves the whole-matrix figure by, at M = 1000


def test_one_element_off_by_4_bf16_ulps_is_flagged_by_the_elementwise_check():
    """(The element of row 123 with the largest magnitude: 4 ulps of an element near zero are below the accumulation term of
    the bound, and rightly so -- an fp32 sum of 320 terms may be that far off there.)"""
    c, guard = _clean(K1=320)
    col = int(guard.view[123].float().abs().argmax())
    v = guard.view[123, col].clone()
    guard.view[123, col] = (v.view(torch.int16) + 4).view(BF)
    res = G.run_checks(c, guard.view, guard)
    assert G.failures(res) == ["elementwise"] and res["violations"] == 1, res
    assert (res["first_violation"]["row"], res["first_violation"]["col"]) == (123, col)
    assert res["rel"] < G.TOL_ONE_ROUNDING                                  # the whole-matrix gate alone passes it


def test_one_element_of_an_fp32_output_off_in_the_fourth_digit_is_flagged():
    c, guard = _clean(M=257, N=72, K1=32, dtype=F32)
    col = int(guard.view[200].abs().argmax())
    guard.view[200, col] *= 1.0 + 1e-4
    res = G.run_checks(c, guard.view, guard)
    assert G.failures(res) == ["elementwise"] and res["violations"] == 1, res
    assert res["rel"] < G.TOL_F32                                           # the fp32 gate alone passes it


@pytest.mark.parametrize("where", ["guard_row_before", "guard_row_after", "pad_column"])
def test_a_store_past_the_edge_is_flagged_by_the_canary(where):
    c, guard = _clean(M=129, N=72, K1=96)
    g = G.GUARD_ROWS
    if where == "guard_row_before":
        guard.buf[g - 1, 5] = 1.0
    elif where == "guard_row_after":
        guard.buf[g + 129, :8] = guard.view[128, :8]                   # the row after the last, 8 columns
    else:
        guard.buf[g + 17, 72:80] = 0.0                                  # 8 columns past the edge of one row
    res = G.run_checks(c, guard.view, guard)
    assert G.failures(res) == ["canary"], res
    assert (res["pad_elems"] == 8) if where == "pad_column" else (res["guard_rows"] == 1), res


def test_a_row_left_unwritten_is_flagged_by_the_canary():
    c, guard = _clean(M=129, N=72, K1=96)
    guard.view[128] = float("nan")
    res = G.run_checks(c, guard.view, guard)
    assert "canary" in G.failures(res) and res["nan_left"] == 72, res
    assert "elementwise" in G.failures(res) and res["violations"] == 72      # (a NaN is also outside every bound)


def test_operand_pads_keep_the_values_and_differ_from_the_output_stride():
    t = torch.randn(5, 64).to(BF)
    p = G.padded(t, G.PAD_A1)
    assert torch.equal(p, t) and p.stride(0) == 128 and float(p.as_strided((5, 128), (128, 1))[0, 64]) == G.PAD_FILL
    assert len({G.PAD_COLS, G.PAD_A1, G.PAD_A2, G.PAD_RES, G.PAD_RB}) == 5
