"""csrc/dto_tdb_mfma_layout.h from plain C++: a stand-alone program is compiled with g++ against the header (and dto_tdb_scheme.h;
no HIP, no engine header), run without a GPU, and the scratch slot it prints is checked for every combination of
n in {65, 72, 128, 160, 256}, m in {1, 3, 7}, both orders, n_mod in {0, 2, 12} that the coefficient table takes:

  * members 2 .. 8, need 0 .. 2: against tests/tdb_share_cases.slot_doubles (DESIGN 4.22's formula, which the launch counts of
    tests/test_gpu_tdb_persistent.py rest on);
  * one member, need 0 .. 4: against `lone_slot_doubles` below, the slot of a lone integrator as the engine had it before the lone
    and the group form became one kernel (written from that formula, not from the header).

Integers, so equality is exact."""
import os
import shutil
import subprocess

import pytest

import tdb_share_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "directtrajopt.jl_amd", "csrc")

NS, MS, ORDERS, MODS = (65, 72, 128, 160, 256), (1, 3, 7), (0, 1), (0, 2, 12)

PROGRAM = r"""
#include <cstdio>
#include "dto_tdb_mfma_layout.h"
using namespace dto;

int main() {
    const int ns[] = {65, 72, 128, 160, 256}, ms[] = {1, 3, 7}, mods[] = {0, 2, 12};
    for (int n : ns)
        for (int m : ms)
            for (int order = 0; order < 2; ++order)
                for (int nmod : mods) {
                    if (!tdb_table_fits(m, order, nmod)) { printf("refused %d %d %d %d\n", n, m, order, nmod); continue; }
                    for (int members = 1; members <= 8; ++members)
                        for (int need = 0; need <= (members == 1 ? 4 : 2); ++need) {
                            const TdbmLayout L = tdbm_layout(n, m, order, nmod, need, members);
                            printf("slot %d %d %d %d %d %d %zu %zu %d %d\n", n, m, order, nmod, need, members, L.total, L.oCoef, L.Ctot, L.ucols);
                        }
                }
    return 0;
}
"""


def lone_slot_doubles(n, m, order, n_mods, need):
    """Slot of a lone integrator: four column sets of np x Ctot, M0, Q x ucols vectors, a 32-column ubar tile in EVERY call (need 4
    uses one column of it), the coefficient table; rounded up to an even count.  need 3: J w (x, d), need 4: J' w (x, x_b)."""
    pad32 = lambda v: (v + 31) // 32 * 32
    np_, p, Q = pad32(n), m + 2 + (m if order else 0), (m + 1) * (1 + n_mods)
    P2 = p * (p + 1) // 2
    C = {0: 1, 1: 1 + p, 2: 1 + p + P2, 3: 2, 4: 1 + p}[need]
    Ctot = pad32(C) + (np_ if need == 1 else 0)
    ucols = 32 if need == 2 else 1
    total = 4 * np_ * Ctot + np_ * np_ + Q * ucols * np_ + 32 * np_ + (1 + p + P2) * Q
    return total + total % 2


def table_fits(m, order, n_mods):
    p = m + 2 + (m if order else 0)
    return (1 + p + p * (p + 1) // 2) * (m + 1) * (1 + n_mods) <= 6144


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    assert shutil.which("g++") is not None, "g++ is needed (the engine's own build needs a C++ compiler too)"
    tmp = tmp_path_factory.mktemp("tdb_mfma_layout")
    src, exe = str(tmp / "layout.cpp"), str(tmp / "layout")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    rows = [l.split() for l in out.splitlines()]
    slots = {tuple(int(v) for v in r[1:7]): int(r[7]) for r in rows if r[0] == "slot"}
    refused = {tuple(int(v) for v in r[1:]) for r in rows if r[0] == "refused"}
    return slots, refused


def _combos():
    return [(n, m, o, c) for n in NS for m in MS for o in ORDERS for c in MODS]


def test_the_header_refuses_what_the_table_check_refuses(layout):
    slots, refused = layout
    want = {k for k in _combos() if not table_fits(*k[1:])}
    assert refused == want and 0 < len(want) < len(_combos())
    assert len(slots) == (len(_combos()) - len(want)) * (5 + 7 * 3)


def test_group_slots_are_design_4_22s(layout):
    slots, _ = layout
    for n, m, o, c in _combos():
        if not table_fits(m, o, c):
            continue
        for members in range(2, 9):
            for need in range(3):
                assert slots[(n, m, o, c, need, members)] == S.slot_doubles(n, m, o, c, need, members), (n, m, o, c, need, members)


def test_one_member_slots_are_the_lone_integrators(layout):
    slots, _ = layout
    for n, m, o, c in _combos():
        if not table_fits(m, o, c):
            continue
        for need in range(5):
            assert slots[(n, m, o, c, need, 1)] == lone_slot_doubles(n, m, o, c, need), (n, m, o, c, need)
