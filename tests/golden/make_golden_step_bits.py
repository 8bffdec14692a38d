"""Bit patterns of the optimizer step's and the loss' kernels, recorded from a build of ANOTHER commit (its parent, when the
kernels are rewritten) through the C ABI alone.  Needs a GPU.

    CTRLORA_LIB=/path/to/that/build/libctrlora_hip.so python tests/golden/make_golden_step_bits.py <commit hash of that build>

writes tests/golden/step_bits.pt (under 200 KB).  The cases, the seeded CPU inputs and the runner are tests/step_bits_ref.py's:
cl_adamw, cl_adamw_dev, cl_adamw_dev_clip and cl_adamw_dev_groups at n = 1, 1000, 64 * 33 and 2^20 + 64 and steps 1, 2 and 1000;
cl_p_losses_mse and cl_p_losses_w at B = 3, per = 1000.  Stored:

    meta     commit (the argument), hipcc (`hipcc --version` where the fixture was recorded: the compiler that the recording build
             most likely came from), inputs (one SHA-256 over every seeded input), torch (its version)
    cases    {case: {output: SHA-256 of the int32 bit pattern}}
    blobs    {SHA-256: int32 tensor}, each distinct pattern once, for the cases step_bits_ref.keeps_pattern() names; the largest
             size and the sizes another size already covers with tensors are held by their digests alone

CTRLORA_LIB is required: recording from the in-tree library would compare the code under test with itself.
"""
import os
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)


def main():
    if len(sys.argv) != 2 or not os.environ.get("CTRLORA_LIB"):
        sys.exit(__doc__)
    from ctrlora_amd import hip            # ctypes loader of $CTRLORA_LIB with the header's argument types; no wrapper is called
    from tests import step_bits_ref as S
    assert torch.cuda.is_available(), "recording needs a GPU"
    L = hip.lib()
    res = S.run_cases(L, hip.stream())
    cases, blobs = {}, {}
    for case, outs in res.items():
        cases[case] = {}
        for name, pattern in outs.items():
            digest = S.sha(pattern)
            cases[case][name] = digest
            if S.keeps_pattern(case):
                blobs.setdefault(digest, pattern.clone())
    ver = subprocess.run(["hipcc", "--version"], capture_output=True, text=True).stdout.strip().splitlines()
    meta = dict(commit=sys.argv[1], hipcc=next((ln for ln in ver if "HIP version" in ln), ver[0] if ver else "unknown"),
                inputs=S.inputs_digest(), torch=torch.__version__)
    path = os.path.join(HERE, "step_bits.pt")
    torch.save(dict(meta=meta, cases=cases, blobs=blobs), path)
    size = os.path.getsize(path)
    print(f"wrote {path} ({size} bytes): {len(cases)} cases, {len(blobs)} stored patterns, from {meta['commit']} ({meta['hipcc']})")
    assert size < 200 * 1024, size


if __name__ == "__main__":
    main()
