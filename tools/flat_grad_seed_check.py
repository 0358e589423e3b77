"""CPU check of the seeds of tests/test_flat_grad_paths_gpu.py, with the oracle alone (no GPU, no HIP kernel).

For every scenario: the oracle in fp32 stands in for the run under test and supplies the LeakyReLU branches; the fp64 oracle on
those branches must meet the caps the GPU tests assert (flips <= 1e-5 of the elements, flip margin <= 2e-6), and the smallest
|pre-activation| / max of the fp64 run says how far the input is from a flip in ANY fp32 evaluation.  It also prints, per scenario,
the distance between the fp64 and the fp32 oracle on the same branches (worst parameter, max |a - b| / max |b|): the eps32 figure
a `4 x eps32` bar would start from.

    python tools/flat_grad_seed_check.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import torch                                   # noqa: E402

import flat_grad_ref as R                      # noqa: E402
from oracle_step import LreluMargin            # noqa: E402


def main():
    out = {}
    D = R.discriminator()
    for name in R.D_SCENARIOS:
        passes, scales = R.d_scenario(name)
        masks = [R.d_branches(D, p) for p in passes]
        with LreluMargin() as lm:                                 # (the fp64 run on its own branches)
            R.d_truth(D, passes, [None] * len(passes), scales)
        t64 = R.d_truth(D, passes, masks, scales)                 # (asserts the caps)
        t32 = R.d_truth(D, passes, masks, scales, dtype=torch.float32)
        n, e, _ = R.worst(t32, t64)
        out['D/' + name] = dict(fp64_margin=lm.value, eps32=e, eps32_at=n)
    G = R.generator()
    passes = R.g_scenario(G)
    masks = [R.g_branches(G, p) for p in passes]
    with LreluMargin() as lm:
        R.g_truth(G, passes, [None] * len(passes))
    t64, gt64, _ = R.g_truth(G, passes, masks)
    t32, gt32, _ = R.g_truth(G, passes, masks, dtype=torch.float32)
    n, e, _ = R.worst(t32, t64)
    es = max(R.relmax_t(a, b) for p32, p64 in zip(gt32, gt64) for a, b in zip(p32, p64))
    out['G/two_passes'] = dict(fp64_margin=lm.value, eps32=e, eps32_at=n, eps32_styles=es)
    for k, v in out.items():
        print(k, json.dumps(v))


if __name__ == '__main__':
    main()
