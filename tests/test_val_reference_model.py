"""The reference of the loss-by-band table (tests/val_ref.py) bites, and the host restatement the CPU path runs
(ctrlora_amd.validation.accumulate_bands) has its bits.  No GPU."""
import pytest
import torch

from tests import val_ref as V

IDS = [c["name"] for c in V.CASES]


def test_the_case_table_covers_what_it_claims():
    names = set(IDS)
    for B in (1, 3, 64, 65, 130):
        assert {f"B{B}-nb{nb}-random" for nb in (1, 7, 10, 64)} <= names and f"B{B}-T3-nb3" in names
    assert V.ranges(1000, 10)[0] == (0, 99) and V.ranges(1000, 10)[9] == (900, 999)
    assert V.ranges(1000, 7)[:2] == [(0, 142), (143, 285)] and V.ranges(3, 3) == [(0, 0), (1, 1), (2, 2)]
    e7 = V.edge_timesteps(1000, 7)
    assert {0, 999, -1, 1000, 142, 143, 285, 286, 857} <= set(e7)
    assert {99, 100, 899, 900} <= set(V.edge_timesteps(1000, 10))
    for T, nb in ((1000, 7), (1000, 10), (1000, 64), (3, 3), (1000, 1)):
        for k, (lo, hi) in enumerate(V.ranges(T, nb)):
            assert V.band(lo, T, nb) == k == V.band(hi, T, nb) and (lo == 0 or V.band(lo - 1, T, nb) == k - 1)
        assert V.band(-5, T, nb) == 0 and V.band(T + 5, T, nb) == nb - 1
    assert len(set(IDS)) == len(IDS)


@pytest.mark.parametrize("c", V.CASES, ids=IDS)
def test_unmutated_model_and_host_restatement_have_the_reference_bits(c):
    from ctrlora_amd.validation import accumulate_bands
    ref = V.reference(c["name"])
    assert V.same_bits(V.run(V.model_bands, c), ref)
    x, t, acc0 = V.make_ops(c)
    acc = acc0.clone()
    nv = c["n_valid"]
    out = accumulate_bands(x, t, c["T"], c["nbands"], acc, None if nv is None else torch.tensor([nv], dtype=torch.int32))
    assert out is acc and V.same_bits(acc, ref)
    # the table is consistent with itself: the total row counts what the band rows count
    new = ref - acc0
    assert float(new[:-1, 0].sum()) == float(new[-1, 0]) == (c["B"] if nv is None else min(max(nv, 0), c["B"]))


@pytest.mark.parametrize("mutate", V.MUTATIONS)
def test_every_mutation_is_caught_by_some_case(mutate):
    caught = [c["name"] for c in V.CASES if not V.same_bits(V.run(V.model_bands, c, mutate=mutate), V.reference(c["name"]))]
    print(mutate, len(caught), caught[:8])
    assert caught, f"no case tells the '{mutate}' restatement from the reference"


def test_specific_cases_catch_specific_mutations():
    """The cases written for a mistake catch that mistake (not just some unrelated case)."""
    pairs = {"fp32": "big-among-ones", "edge": "edges-nb10", "reverse": "B130-nb10-random", "ignore_n_valid": "B65-nvalid1",
             "overwrite": "B64-nb10-random", "nan_leak": "nan-and-inf"}
    for mutate, name in pairs.items():
        assert not V.same_bits(V.run(V.model_bands, V.CASE[name], mutate=mutate), V.reference(name)), (mutate, name)


def test_non_finite_samples_stay_in_their_band_and_the_total():
    c = V.CASE["nan-and-inf"]
    x, t, acc0 = V.make_ops(c)
    ref = V.reference(c["name"])
    bad = {V.band(int(t[i]), c["T"], c["nbands"]) for i in range(c["B"]) if not torch.isfinite(x[i])} | {c["nbands"]}
    for k in range(c["nbands"] + 1):
        assert bool(torch.isfinite(ref[k]).all()) == (k not in bad), k


def test_fp32_accumulation_would_lose_the_ones():
    c = V.CASE["big-among-ones"]
    ref = V.reference(c["name"])
    assert float(ref[-1, 1]) == 1e8 + (c["B"] - 1) and float(ref[-1, 0]) == c["B"]
    assert float(V.run(V.model_bands, c, mutate="fp32")[-1, 1]) != float(ref[-1, 1])
