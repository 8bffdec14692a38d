"""The bits of the optimizer step's and the loss' kernels against a record of ANOTHER build: tests/golden/step_bits.pt holds the
int32 bit patterns (or, for the larger sizes, their SHA-256) of every output of cl_adamw, cl_adamw_dev, cl_adamw_dev_clip,
cl_adamw_dev_groups, cl_p_losses_mse and cl_p_losses_w on seeded inputs, recorded through the C ABI from a build of the commit named
in the fixture -- the last one in which each of those entry points had a kernel of its own.  csrc/elementwise.hip now writes the
AdamW update and the p_losses kernel pair once, so tests/test_gpu_optim_groups.py (grouped against one-group), test_adamw_dev_clip
(coefficient 1.0 against cl_adamw_dev) and tests/test_gpu_loss_conformance.py (no table, l2 against cl_p_losses_mse) compare an
expression with itself; this fixture carries what they used to prove.  Cases, inputs and the runner: tests/step_bits_ref.py.

The runner also asserts that g, the hyper table, the map, the loss' inputs and the 64-float guards around every buffer are
untouched.  Nothing here skips on a compiler or torch version: a mismatch fails and says how to regenerate.
"""
import os

import pytest
import torch

from tests import step_bits_ref as S
from tests.util import ROOT

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(ROOT, "tests", "golden", "step_bits.pt")
_RUN = {}


def _golden():
    return torch.load(FIXTURE, map_location="cpu", weights_only=False)


def _results():
    """Every case once, shared by the tests below."""
    if not _RUN:
        if not torch.cuda.is_available():
            pytest.skip("needs a GPU")
        from ctrlora_amd import hip
        _RUN.update(S.run_cases(hip.lib(), hip.stream()))
    return _RUN


def _how(meta):
    return (f"tests/golden/step_bits.pt was recorded from commit {meta['commit']} ({meta['hipcc']}, torch {meta['torch']}).  If the "
            f"change of bits is intended, record it again from a build of the commit to compare with: CTRLORA_LIB=<that build's "
            f"libctrlora_hip.so> python tests/golden/make_golden_step_bits.py <its commit hash>")


def _mismatches(gold, res, prefix):
    bad = []
    for case, outs in gold["cases"].items():
        if not case.startswith(prefix):
            continue
        for name, digest in outs.items():
            got = res[case][name]
            if S.sha(got) == digest:
                continue
            want = gold["blobs"].get(digest)
            if want is None:
                bad.append(f"{case} {name}: digest differs ({got.numel()} elements, pattern not stored)")
            else:
                assert want.shape == got.shape, (case, name, want.shape, got.shape)
                bad.append(f"{case} {name}: {int((want != got).sum())} of {got.numel()} elements differ")
    return bad


def test_fixture_holds_every_case_and_the_seeded_inputs_are_the_recorded_ones():
    gold = _golden()
    want = {c[0] for c in S.adamw_cases()} | {c[0] for c in S.loss_cases()}
    assert set(gold["cases"]) == want and len(want) == 60 + 6
    assert all(set(o) == {"p", "m", "v"} for c, o in gold["cases"].items() if c.startswith("adamw"))
    assert all(set(o) == {"d_eps", "out", "per_sample", "scratch"} for c, o in gold["cases"].items() if c.startswith("p_losses"))
    for case, outs in gold["cases"].items():
        for name, digest in outs.items():
            assert (digest in gold["blobs"]) == S.keeps_pattern(case), (case, name)
    assert all(b.dtype == torch.int32 and S.sha(b) == d for d, b in gold["blobs"].items())
    assert len(gold["meta"]["commit"]) == 40 and "HIP version" in gold["meta"]["hipcc"]
    assert os.path.getsize(FIXTURE) < 200 * 1024
    assert S.inputs_digest() == gold["meta"]["inputs"], \
        "the seeded CPU generators draw other numbers than when the fixture was recorded: no kernel is at fault.  " + _how(gold["meta"])


@pytest.mark.parametrize("entry", ["adamw/", "adamw_dev/", "adamw_dev_clip/", "adamw_dev_groups/", "p_losses_mse/", "p_losses_w/"])
def test_entry_point_reproduces_the_recorded_bits(entry):
    gold = _golden()
    res = _results()
    assert S.inputs_digest() == gold["meta"]["inputs"], "the seeded inputs are not the recorded ones.  " + _how(gold["meta"])
    assert any(c.startswith(entry) for c in gold["cases"])
    bad = _mismatches(gold, res, entry)
    assert not bad, f"{len(bad)} outputs differ from the record:\n  " + "\n  ".join(bad) + "\n" + _how(gold["meta"])


def test_the_record_says_what_the_deleted_comparisons_said():
    """Within the record itself: a clip coefficient of 1.0 has cl_adamw_dev's bits, cl_p_losses_w without a table and with l2 has
    cl_p_losses_mse's, the moments do not depend on the step, and the clip and the table act."""
    c = _golden()["cases"]
    for n in S.SIZES:
        for step in S.STEPS:
            assert c[f"adamw_dev_clip/n{n}/s{step}/c1.0"] == c[f"adamw_dev/n{n}/s{step}"]
            assert c[f"adamw_dev_clip/n{n}/s{step}/c{S.COEF}"]["p"] != c[f"adamw_dev/n{n}/s{step}"]["p"]
            assert {k: c[f"adamw_dev/n{n}/s{step}"][k] for k in "mv"} == {k: c[f"adamw_dev/n{n}/s1"][k] for k in "mv"}
        assert len({c[f"adamw_dev/n{n}/s{step}"]["p"] for step in S.STEPS}) == 3
    assert c["p_losses_w/no_table/l2"] == c["p_losses_mse/lvlb"]
    assert len({c[k]["d_eps"] for k in c if k.startswith("p_losses_w")}) == 4
    assert c["p_losses_mse/lvlb"]["d_eps"] == c["p_losses_mse/no_lvlb"]["d_eps"] and c["p_losses_mse/lvlb"]["out"] != c["p_losses_mse/no_lvlb"]["out"]
