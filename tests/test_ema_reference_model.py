"""tests/ema_ref.py against tests/golden/ema.pt (written by the unmodified reference's LitEma: tests/golden/make_golden_ema.py):
the restatement the GPU tests compare cl_ema_update with IS LitEma's arithmetic, bit for bit, and the fixture tells it apart
from its two nearest neighbours.  No GPU."""
import pytest

from tests import ema_ref as E

RUNS = ("defaults", "no_warmup", "crossing")


@pytest.fixture(scope="module")
def fixture():
    return E.load_fixture()


@pytest.mark.parametrize("name", RUNS)
def test_restatement_reproduces_the_reference_bit_for_bit(fixture, name):
    run = fixture[name]
    got, counts = E.replay(run)
    assert counts == run["num_updates"]
    assert len(got) == len(run["shadows"]) == 12
    for k, (mine, want) in enumerate(zip(got, run["shadows"])):
        assert set(mine) == set(want)
        for key in want:
            assert E.same_bits(mine[key], want[key]), (name, k, key)


def test_the_crossing_run_crosses_the_cap(fixture):
    """In exact arithmetic (1 + u) / (10 + u) is below 0.9999 up to u = 89 989 and reaches it at 89 990, inside the run.  In fp32
    the quotient is within half an ulp of the cap over the whole window and rounds to the cap's own fp32 value, so whichever side
    min() takes, the decay has the cap's bits: the run pins the quotient's rounding next to the cap, not a visible switch."""
    from fractions import Fraction
    counts = fixture["crossing"]["num_updates"]
    assert counts[0] == 89986 and counts[-1] == 89997 and counts == list(range(89986, 89998))
    exact = [Fraction(1 + u, 10 + u) < Fraction(9999, 10000) for u in counts]
    assert exact[:4] == [True] * 4 and exact[4:] == [False] * 8, exact
    cap = E.F(0.9999)
    assert all(E.F(1 + u) / E.F(10 + u) == cap and E.decay_at(0.9999, u) == cap for u in counts)
    # far from the cap the warm-up term rules: the defaults run
    assert [float(E.decay_at(0.9999, u)) for u in (1, 2)] == [float(E.F(2) / E.F(11)), float(E.F(3) / E.F(12))]
    assert E.decay_at(0.9, -1) == E.F(0.9) and E.decay_at(0.5, 100) == E.F(0.5)
    assert fixture["no_warmup"]["num_updates"] == [-1] * 12 and fixture["defaults"]["num_updates"] == list(range(1, 13))


@pytest.mark.parametrize("near_miss", [E.update_contracted, E.update_lerp], ids=["fma-contracted", "d*s+omd*p"])
def test_the_fixture_bites(fixture, near_miss):
    differing = 0
    for name in RUNS:
        run = fixture[name]
        got, _ = E.replay(run, near_miss)
        differing += sum(int((E.bits(got[k][key]) != E.bits(run["shadows"][k][key])).sum())
                         for k in range(12) for key in run["shadows"][k])
    assert differing >= 1, "the fixture cannot tell this form from LitEma's"


def test_shadow_key_rule_gives_the_fixture_names(fixture):
    from ldm.modules.ema import shadow_key
    for run in fixture.values():
        assert run["names"] == {n: E.shadow_key(n) for n in run["names"]} == {n: shadow_key(n) for n in run["names"]}
        assert "frozen" not in run["names"] and set(run["names"]) == {"bias", "proj.weight", "conv.weight"}
        assert all(set(s) == set(run["names"].values()) for s in run["shadows"])
    assert E.shadow_key("control_model.zero_convs.0.0.weight") == "control_modelzero_convs00weight"
