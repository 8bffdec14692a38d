"""Kernel-level conformance of csrc/attention_causal.hip (cl_attention_causal_fwd): every row of the case table of
tests/attn_causal_ref.py through hip.attention_causal, element-wise against the fp64 causal reference with zero violations, plus
the rel-L2 gate; outputs are NaN-filled views into guarded buffers and every operand a padded copy with a row pitch of its own.
The probe must report the causal family and one workgroup per (64-query block, head, sample); the refusals launch nothing."""
import ctypes

import pytest
import torch

from tests import attn_causal_ref as R
from tests.attn_ref import PROBE_FIELDS
from tests.test_gpu_bench_shapes import _need_gpu, _record

pytestmark = pytest.mark.gpu

PADS = dict(q=8, k=16, v=24)          # row pitches of their own, whole 16-byte units in both dtypes


def _probe():
    from ctrlora_amd import hip
    out = (ctypes.c_int * 16)()
    assert hip.lib().cl_debug_attention_last_launch(out) == 0
    return dict(zip(PROBE_FIELDS, list(out)))


@pytest.mark.parametrize("row", R.CASES, ids=[r["name"] for r in R.CASES])
def test_every_row_meets_the_elementwise_gate(row):
    _need_gpu()
    from ctrlora_amd import hip
    case = R.make_case(row)
    ref = R.causal_ref64(case)
    B, H, N, dt = case["B"], case["H"], case["N"], row["dtype"]
    q, k, v = (R.padded(case[n].cuda(), PADS[n]) for n in "qkv")
    og = R.Guarded(B * N, H * R.DH, dt, "cuda")
    hip.attention_causal(q, k, v, og.view, B, H, N, R.DH, case["scale"])
    probe = _probe()
    torch.cuda.synchronize()
    got = og.view.cpu()
    res = R.check(got, ref, dt)
    print(f"causal {row['name']}: err/bound {res['err_over_bound']:.3f} excess {res['excess']:.3f} rel {res['rel']:.3e}")
    _record("attention_causal", row=row["name"], err_over_bound=res["err_over_bound"], excess=res["excess"], rel=res["rel"],
            violations=res["violations"])
    assert og.check() == dict(guard_rows=0, pad_elems=0, nan_left=0)
    assert res["violations"] == 0, res
    assert res["rel"] < res["rel_gate"], res
    # query row 0 of every head sees one key: v[0], to one output rounding (P = 1 exactly, the product and the quotient exact)
    assert torch.equal(got.reshape(B, N, -1)[:, 0], case["v"].reshape(B, N, -1)[:, 0])
    want = dict(kind=1, family=R.FAM_CAUSAL, dtype=0 if dt == R.BF else 1, dh=64, grid_fwd=(N + 63) // 64 * H * B, tile=64)
    assert {k_: probe[k_] for k_ in want} == want, probe


def test_two_launches_are_bit_identical():
    _need_gpu()
    from ctrlora_amd import hip
    case = R.make_case(R.CASES[6])
    B, H, N = case["B"], case["H"], case["N"]
    outs = []
    for _ in range(2):
        o = torch.empty(B * N, H * R.DH, dtype=case["dtype"], device="cuda")
        hip.attention_causal(case["q"].cuda(), case["k"].cuda(), case["v"].cuda(), o, B, H, N, R.DH, case["scale"])
        outs.append(o)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("dtype", [R.BF, R.F32], ids=["bf16", "f32"])
def test_refusals_return_an_error_and_write_nothing(dtype):
    _need_gpu()
    from ctrlora_amd import hip
    L = hip.lib()
    B, H = 1, 2
    x = torch.zeros(256, 136, dtype=dtype, device="cuda")
    og = R.Guarded(129, 128, dtype, "cuda")
    p, o = x.data_ptr(), og.view.data_ptr()
    d = hip.dt(x)
    call = lambda N=64, dh=64, ldq=136, ldo=136, Q=p, O=o, Hh=H: L.cl_attention_causal_fwd(d, Q, ldq, p, 136, p, 136, O, ldo, B, Hh, N, dh,
                                                                                           0.125, hip.stream())
    odd = 132 if dtype == R.BF else 130                                # 264 / 520 bytes: no multiple of 16
    for name, rc in (("dh 40", call(dh=40, Hh=3)), ("N 0", call(N=0)), ("N 129", call(N=129)), ("odd pitch", call(ldq=odd)),
                     ("odd output pitch", call(ldo=odd)), ("null Q", call(Q=None)), ("null O", call(O=None)),
                     ("pitch below H dh", call(ldq=120)), ("dtype 2", L.cl_attention_causal_fwd(2, p, 136, p, 136, p, 136, o, 136, B, H,
                                                                                                64, 64, 0.125, hip.stream()))):
        assert rc == 1, (name, rc)
        assert _probe()["kind"] == 0, name                             # nothing launched
    torch.cuda.synchronize()
    assert og.check() == dict(guard_rows=0, pad_elems=0, nan_left=129 * 128)
    with pytest.raises(hip.HipError, match="code 1"):                  # and through the wrapper
        hip.attention_causal(x[:80, :80], x[:80, :80], x[:80, :80], og.view[:80, :80], 1, 2, 80, 40, 0.1)
    assert call() == 0 and _probe()["family"] == R.FAM_CAUSAL          # the same call with nothing wrong is taken
    torch.cuda.synchronize()
