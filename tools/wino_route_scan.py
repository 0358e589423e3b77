"""Writes profiles/wino_route_scan.json: how often each branch of the Winograd planners (hg_wino.hip make_plan / make_wg_plan)
is taken over the argument grid of tests/test_wino_route_cpu.py, asked of the built library through hg_wino_route /
hg_wino_wgrad_route (host logic; 256 CUs).  The test asserts that the record still holds.

    python tools/wino_route_scan.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import test_wino_route_cpu as T   # noqa: E402


def main():
    import histogan_amd._lib as L
    assert L.wino_route(32, 256, 128, 64, 64).cus == 256 and not any(k in os.environ for k in T.KNOBS)
    rec = {'what': 'tools/wino_route_scan.py: routes of hg_wino_route / hg_wino_wgrad_route over the grid B x K x N x H x W, '
                   '256 CUs, no HG_WINO_* knob; library version %d' % L.lib.hg_version(),
           'grid': {'B': list(T.BS), 'K': list(T.CH), 'N': list(T.CH), 'H': list(T.HS), 'W': list(T.HS)},
           'counts': T.scan(L)}
    with open(T.RECORD, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print(json.dumps(rec['counts'], indent=1))


if __name__ == '__main__':
    main()
