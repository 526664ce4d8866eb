"""csrc/dto_bgemm_dispatch.h from plain C++: a stand-alone program is compiled with g++ against the header alone (no HIP, no engine
header), run without a GPU, and the kernel, block size and grid it names for a launch are compared with a table worked out by hand
from the launcher the header replaced: grid = ceil8(nbatch) x tiles per matrix, capped at 1024 (64-tile kernel) or 512 (ring kernel)
unless the epilogue is polynomial.  The rows sit on both sides of every branch: npad % 128 != 0, one 128-tile per matrix on both sides
of 3500 intervals, several 128-tiles, grids under and over the cap."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "directtrajopt.jl_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "dto_bgemm_dispatch.h"

// argv: groups of npad nbatch poly force_tile64 ring_persist_all; a group at the defaults goes through the default arguments
int main(int argc, char** argv) {
    for (int i = 1; i + 4 < argc; i += 5) {
        const int npad = atoi(argv[i]), nbatch = atoi(argv[i + 1]), poly = atoi(argv[i + 2]);
        const int force = atoi(argv[i + 3]), all = atoi(argv[i + 4]);
        const dto::BGemmLaunch l = force == -1 && !all ? dto::bgemm_dispatch(npad, nbatch, poly != 0)
                                                        : dto::bgemm_dispatch(npad, nbatch, poly != 0, force, all != 0);
        printf("%s %d %d\n", l.ring ? "ring" : "tile64", l.threads, l.grid);
    }
    return 0;
}
"""

# npad, nbatch, epilogue -> kernel, threads, grid (switches at their defaults: what the product library does)
TABLE = [
    (64, 10, "plain", "tile64", 256, 16),
    (64, 2000, "plain", "tile64", 256, 1024),
    (64, 2000, "poly", "tile64", 256, 2000),
    (128, 3499, "square", "tile64", 256, 1024),
    (128, 3499, "poly", "tile64", 256, 14016),
    (128, 3500, "plain", "ring", 512, 512),
    (128, 3500, "poly", "ring", 512, 3504),
    (192, 100, "poly", "tile64", 256, 936),
    (256, 30, "plain", "ring", 512, 128),
    (256, 2000, "square", "ring", 512, 512),
    (256, 2000, "poly", "ring", 512, 8000),
    (320, 3, "plain", "tile64", 256, 200),
    (1024, 500, "poly", "ring", 512, 32256),
]

# the two switches of TUNING builds: npad, nbatch, epilogue, DTO_BGEMM_TILE64, DTO_BGEMM_RING == 1 -> kernel, threads, grid
SWITCHED = [
    (256, 2000, "plain", 1, 0, "tile64", 256, 1024),    # forced onto 64-tiles: ceil8(2000) x 16 slots, persistent
    (256, 2000, "poly", 1, 0, "tile64", 256, 32000),
    (128, 100, "plain", 0, 0, "ring", 512, 104),        # forced off them below the crossover
    (192, 100, "plain", 0, 0, "tile64", 256, 936),      # no whole 128-tiles: the ring kernel cannot run, whatever is forced
    (256, 2000, "poly", -1, 1, "ring", 512, 512),       # everything persistent
    (128, 100, "poly", -1, 1, "tile64", 256, 416),      # ... says nothing about the 64-tile kernel
]


@pytest.fixture(scope="module")
def dispatch(tmp_path_factory):
    assert shutil.which("g++") is not None, "g++ is needed (the engine's own build needs a C++ compiler too)"
    tmp = tmp_path_factory.mktemp("bgemm_dispatch")
    src, exe = str(tmp / "dispatch.cpp"), str(tmp / "dispatch")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe], check=True)

    def ask(rows):
        args = [str(v) for r in rows for v in r]
        out = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout
        got = [(k, int(t), int(g)) for k, t, g in (l.split() for l in out.splitlines())]
        assert len(got) == len(rows)
        return got
    return ask


def test_default_dispatch_matches_the_hand_derived_table(dispatch):
    got = dispatch([(npad, nb, int(epi == "poly"), -1, 0) for npad, nb, epi, *_ in TABLE])
    for row, g in zip(TABLE, got):
        print(row, g)
        assert g == row[3:], (row, g)


def test_accuracy_budget_fixtures_reach_the_kernel_their_case_names(dispatch):
    """tests/hp_cases.py: with six intervals the 250- and 330-state fixtures run the chain on the ring kernel, whatever the
    epilogue; the 130-state one (npad 192: no whole 128-tiles) and the 66-state one (npad 128, far below 3500 intervals) do not."""
    import sys
    sys.path[:0] = [p for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")) if p not in sys.path]
    import hp_cases as C
    want = {"hp_general": (128, "tile64"), "hp_tile192": (192, "tile64"), "hp_ring256": (256, "ring"),
            "hp_ring256_q1": (256, "ring"), "hp_ring384": (384, "ring")}
    nb = C.N_KNOTS - 1
    for name, (npad, kernel) in want.items():
        assert -(-C.CASES[name]["n"] // 64) * 64 == npad, name
        got = dispatch([(npad, nb, poly, -1, 0) for poly in (0, 1)])
        assert [g[0] for g in got] == [kernel, kernel], (name, got)


def test_forced_tile_and_all_persistent_ring(dispatch):
    got = dispatch([(npad, nb, int(epi == "poly"), force, ring) for npad, nb, epi, force, ring, *_ in SWITCHED])
    for row, g in zip(SWITCHED, got):
        print(row, g)
        assert g == row[5:], (row, g)
