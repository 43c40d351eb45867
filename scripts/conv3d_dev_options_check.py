"""Development aid (no GPU needed): the development switches that act on the launch plan of dmb_conv3d_k3_f32 -- options 2, 3, 10, 13,
19 and 23 -- each force the plan code they name, and with every option back at 0 the recorded codes of
tests/test_conv3d_plan_host.py return.  One process on the development library (python -m densematchingbenchmark_amd.build --dev):
    python scripts/conv3d_dev_options_check.py > profiles/conv3d_retire_dev_options.log"""
import os
os.environ.setdefault("DMB_LIB", "dev")
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from densematchingbenchmark_amd import _lib
from test_conv3d_plan_host import CASES, NCU

lib = _lib.load()
ROWS = {c[0]: c for c in CASES}
bad = 0


def check(row, opts, want):
    """`want`: the code the options force, or a set of codes (option 13: the estimate's pick among the box tiles)"""
    global bad
    for k, v in opts:
        lib.dmb_dev_set_option(k, v)
    got = lib.dmb_conv3d_k3_plan(*ROWS[row][1:12], NCU)
    for k, _ in opts:
        lib.dmb_dev_set_option(k, 0)
    ok = got in want if isinstance(want, set) else got == want
    bad += not ok
    print("%-34s %-12s -> %#06x   (recorded %#06x)   %s" % (row, ", ".join("%d = %d" % o for o in opts) or "all 0", got, ROWS[row][12],
                                                          "ok" if ok else "WRONG, expected " + str(want)))


S1_32, S1_64, S2_64, SK, NO_SK = "s1 32 headline", "s1 64 runs (quarter resolution)", "s2 64 four rows", "split-K s1 64->64", "split-K s1 390 chains"
for k in (1, 2, 3, 4):        # 19 = k: candidate k - 1 of S1Tiles32
    check(S1_32, [(19, k)], 0x200 + k - 1)
for k in (1, 2, 3, 4, 5):     # ... of S1Tiles64
    check(S1_64, [(19, k)], 0x204 + k - 1)
check(S1_32, [(2, 1)], 0x300)             # flattened tiles (240 and 60 columns: TX 60)
check(S1_64, [(2, 1)], 0x302)
check(S1_64, [(13, 1)], {0x205, 0x206, 0x207, 0x208})   # boxes instead of runs
check(S1_64, [(13, 1), (19, 1)], {0x205, 0x206, 0x207, 0x208})
check(S2_64, [(3, 1)], 0x505)             # dword staging
check(S2_64, [(10, 2)], 0x504)            # dword epilogue
check(S2_64, [(10, 3)], 0x500)            # one-row tiles
check(S2_64, [(10, 4)], 0x501)            # two-row tiles
check(SK, [(23, 1)], 0x208)               # split-K never: the row's full-grid plan
check(SK, [(23, 2)], 0x101)               # split-K variant 1 forced
check(NO_SK, [(23, 2)], 0x101)            # ... where the estimate declines it
check(NO_SK, [(23, 3)], 0x203)            # a variant the build does not hold: the full-grid plan
for c in CASES:               # everything back at 0
    got = lib.dmb_conv3d_k3_plan(*c[1:12], NCU)
    bad += got != c[12]
    if got != c[12]:
        print("%-34s all 0 -> %#06x   WRONG, recorded %#06x" % (c[0], got, c[12]))
print("all options 0: %d recorded rows of tests/test_conv3d_plan_host.py checked" % len(CASES))
print("failures: %d" % bad)
sys.exit(1 if bad else 0)
