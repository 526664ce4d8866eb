"""CPU checks of the preconditioned step's boundary (include/dto_engine.h, "Preconditioned truncated-Newton step"): the eight entry
points are declared, exported and typed alike in the header, the ctypes table and the Julia file; a structure-only handle, which needs
no GPU, refuses with text and stays usable; a push or a harvest without capacity, a capacity outside 0 .. 16, a non-finite entry of a
pushed pair, every bad argument of the step and every overlap of an output with an input are refused with text, and nothing is
written."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dto_amd
import dto_oracle as O
from helpers import to_engine
from test_newton_abi import BAD, c_kind, header_source, header_text, julia_source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Z, sigma, mu, rho, free_mask, lo, hi, radius, shift, rtol, atol, max_iter, harvest, p, info, trace, entry_state, Zp
STEP = ["handle", "ptr", "double", "ptr", "ptr", "ptr", "ptr", "ptr", "double", "double", "double", "double", "int32", "int32", "ptr", "ptr", "ptr",
        "ptr", "ptr"]
KINDS = {
    "dto_newton_pairs_push": ["handle", "ptr", "ptr"],                              # s, y
    "dto_newton_precondition": ["handle", "ptr", "int32", "ptr", "ptr"],            # free_mask, n_cols, r, z
    "dto_preconditioned_newton_step": STEP,
}
NAMES = [n + s for n in KINDS for s in ("", "_dev")]
PLAIN = {"dto_newton_pairs_clear": ["handle"], "dto_newton_pairs_info": ["handle", "int32_ptr", "int32_ptr"]}


def kinds_of(name):
    if name in PLAIN:
        return PLAIN[name]
    return KINDS[name[:-4]] + ["stream"] if name.endswith("_dev") else KINDS[name]


def kind(arg):
    arg = " ".join(arg.split())
    return "int32_ptr" if re.fullmatch(r"int32_t\* \w+", arg) else c_kind(arg)


def test_the_eight_names_are_declared_and_typed():
    src = header_source()
    for n in NAMES + list(PLAIN):
        m = re.search(r"\bint\s+" + n + r"\s*\(([^)]*)\)\s*;", src)
        assert m, f"{n} is not declared"
        assert [kind(a) for a in m.group(1).split(",")] == kinds_of(n), n
    assert re.search(r"#define\s+DTO_ABI_VERSION\s+8\b", src) and dto_amd.capi.DTO_ABI_VERSION == 8, "additions only: the version stays"


def test_the_ctypes_prototypes_are_typed_like_the_header():
    host = {"handle": C.c_void_p, "ptr": dto_amd.capi.c_double_p, "double": C.c_double, "int32": C.c_int32, "int32_ptr": dto_amd.capi.c_int32_p}
    dev = dict(host, ptr=C.c_void_p, stream=C.c_void_p)
    for n in NAMES + list(PLAIN):
        res, args = dto_amd.capi.SYMBOLS[n]
        assert res is C.c_int
        table = dev if n.endswith("_dev") else host
        assert list(args) == [table[k] for k in kinds_of(n)], n


def test_the_julia_file_names_every_entry_point_typed_like_the_header():
    src = julia_source()
    jl = {"handle": "Ptr{Cvoid}", "ptr": "Ptr{Float64}", "double": "Float64", "int32": "Int32", "stream": "Ptr{Cvoid}", "int32_ptr": "Ptr{Int32}"}
    for n in NAMES + list(PLAIN):
        m = re.search(r"@ccall\s+lib\." + n + r"\((.*?)\)::Cint", src, flags=re.S)
        assert m, f"{n} has no @ccall"
        types = [a.strip().split("::")[-1] for a in m.group(1).split(",")]
        assert types == [jl[k] for k in kinds_of(n)], (n, types)
    for f in ("newton_pairs_push!", "newton_pairs_push_dev!", "newton_pairs_clear!", "newton_pairs_info", "newton_precondition", "newton_precondition_dev!",
              "preconditioned_newton_step", "preconditioned_newton_step_dev!"):
        assert re.search(r"^(function )?" + re.escape(f) + r"\(", src, flags=re.M), f


def test_the_header_section_the_plan_header_and_the_profile_name():
    text = header_text()
    a, b, c = text.index("---- Augmented-Lagrangian terms"), text.index("---- Preconditioned truncated-Newton step"), text.index("---- Multi-GPU")
    assert a < b < c
    section = text[b:c]
    for n in NAMES + list(PLAIN):
        assert re.search(r"\bint\s+" + n + r"\s*\(", section), n
    for word in ("Morales", "Byrd", "newton_pairs", "two banks", "admitted", "2^-26", "gamma", "harvest", "Fallback", "info [16]", "[max_iter][8]",
                 "Euclidean", "bit for bit", "Refused with text", "rounded on its own", "principal submatrix"):
        assert word in section, word
    assert '"precond"' in text[text.index("int dto_profile_enable"):] and '"newton_pairs"' in text[c:], "the profile name and the option are listed"
    plan = open(os.path.join(ROOT, "directtrajopt.jl_amd", "csrc", "dto_precond_plan.h")).read()
    assert '#include "dto_newton_box_plan.h"' in plan and "hip" not in re.sub(r"//.*", "", plan).lower().replace("__hipcc__", "")
    assert "dto_precond.$(O)" in open(os.path.join(ROOT, "Makefile")).read()


def test_the_library_exports_them(engine_lib):
    lib = os.path.join(ROOT, "directtrajopt.jl_amd", "libdto_engine.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for n in NAMES + list(PLAIN):
        assert n in exported, f"{n} is not exported"
        assert hasattr(engine_lib, n)


@pytest.fixture()
def structure_only():
    ev = dto_amd.Evaluator(to_engine(O.make_scaled_problem(5, 6, 2, seed=4, with_constraint=True)), device=-1)
    yield ev
    ev.close()


def test_a_structure_only_handle_refuses_with_text_and_stays_usable(structure_only):
    ev = structure_only
    n, m = ev.n_variables, ev.n_constraints
    Z, mu = np.zeros(n), np.zeros(m)
    assert ev.newton_pairs_info() == (0, 0), "the default capacity is 0: off"
    ev.set_option("newton_pairs", 4)
    assert ev.newton_pairs_info() == (0, 4)
    for call in (lambda: ev.preconditioned_newton_step(Z),
                 lambda: ev.preconditioned_newton_step(Z, 0.7, mu, np.full(m, 10.0), lo=np.full(n, -1.0), hi=np.ones(n), free=np.ones(n), radius=1.0,
                                                       shift=2.0, max_iter=3, harvest=True, trace=True, states=True, trajectory=True),
                 lambda: ev.preconditioned_newton_step_dev(8, 1.0, 0, 0, 0, 0, 0, 0.0, 0.0, 1e-6, 0.0, 5, True, 8 + 8 * n, 8 + 16 * n),
                 lambda: ev.newton_pairs_push(np.ones(n), np.ones(n)),
                 lambda: ev.newton_pairs_push_dev(8, 8 + 8 * n),
                 lambda: ev.newton_precondition(np.ones(n)),
                 lambda: ev.newton_precondition(np.ones((3, n)), free=np.ones(n)),
                 lambda: ev.newton_precondition_dev(0, 2, 8, 8 + 16 * n)):
        with pytest.raises(dto_amd.EngineError, match="structure-only"):
            call()
    ev.newton_pairs_clear()
    assert ev.newton_pairs_info() == (0, 4)
    rows, cols = ev.jacobian_structure()
    assert rows.size == ev.n_jacobian_entries == cols.size
    with pytest.raises(ValueError, match="wrong length"):
        ev.preconditioned_newton_step(Z[:-1])
    for word in ("free", "lo", "hi"):
        with pytest.raises(ValueError, match=word):
            ev.preconditioned_newton_step(Z, **{word: np.ones(3)})
    for word in ("s", "y"):
        with pytest.raises(ValueError, match=word):
            ev.newton_pairs_push(**dict(dict(s=np.ones(n), y=np.ones(n)), **{word: np.ones(3)}))
    with pytest.raises(ValueError, match="r"):
        ev.newton_precondition(np.ones((2, n - 1)))


def test_a_push_or_a_harvest_without_capacity_and_a_capacity_out_of_range_are_refused(structure_only):
    ev = structure_only
    n = ev.n_variables
    Z = np.zeros(n)
    with pytest.raises(dto_amd.EngineError, match="dto_newton_pairs_push: the pair store has no capacity.*newton_pairs"):
        ev.newton_pairs_push(np.ones(n), np.ones(n))
    with pytest.raises(dto_amd.EngineError, match="dto_newton_pairs_push_dev: the pair store has no capacity"):
        ev.newton_pairs_push_dev(8, 8 + 8 * n)
    with pytest.raises(dto_amd.EngineError, match="dto_preconditioned_newton_step: harvest needs a pair store.*newton_pairs") as e:
        ev.preconditioned_newton_step(Z, harvest=True)
    assert "structure-only" not in str(e.value)
    with pytest.raises(dto_amd.EngineError, match="dto_preconditioned_newton_step_dev: harvest needs a pair store"):
        ev.preconditioned_newton_step_dev(8, 1.0, 0, 0, 0, 0, 0, 0.0, 0.0, 1e-6, 0.0, 5, True, 8 + 8 * n, 8 + 16 * n)
    with pytest.raises(dto_amd.EngineError, match="structure-only"):
        ev.preconditioned_newton_step(Z, harvest=False)
    for bad in (-1, 17, 1 << 40):
        with pytest.raises(dto_amd.EngineError, match=r"newton_pairs takes 0 \(no preconditioner\) \.\. 16"):
            ev.set_option("newton_pairs", bad)
    assert ev.newton_pairs_info() == (0, 0)
    for good in (16, 1, 0):
        ev.set_option("newton_pairs", good)
        assert ev.newton_pairs_info() == (0, good)


def test_a_non_finite_entry_of_a_pushed_pair_is_named(structure_only):
    ev = structure_only
    n = ev.n_variables
    ev.set_option("newton_pairs", 2)
    for bad in (np.inf, -np.inf, np.nan):
        s, y = np.ones(n), np.ones(n)
        s[n - 1] = bad
        with pytest.raises(dto_amd.EngineError, match=rf"dto_newton_pairs_push: s\[{n - 1}\] is not finite") as e:
            ev.newton_pairs_push(s, y)
        assert "structure-only" not in str(e.value)
        with pytest.raises(dto_amd.EngineError, match=r"dto_newton_pairs_push: y\[0\] is not finite"):
            ev.newton_pairs_push(np.ones(n), np.where(np.arange(n) == 0, bad, 1.0))
    assert ev.newton_pairs_info() == (0, 2)
    dp = lambda a: None if a is None else a.ctypes.data_as(dto_amd.capi.c_double_p)
    for s_, y_ in ((None, np.ones(n)), (np.ones(n), None)):
        assert ev._lib.dto_newton_pairs_push(ev._h, dp(s_), dp(y_)) != 0 and "NULL" in ev._lib.dto_last_error(ev._h).decode()


@pytest.mark.parametrize("kw,word", BAD, ids=[f"{list(k)[0]}={list(k.values())[0]}" for k, _ in BAD])
def test_what_the_extended_calls_refuse_is_refused_with_text(structure_only, kw, word):
    """the arguments are judged before the handle is: a structure-only handle names the bad one (a good call says "structure-only")"""
    ev = structure_only
    n = ev.n_variables
    Z = np.zeros(n)
    with pytest.raises(dto_amd.EngineError, match=word) as e:
        ev.preconditioned_newton_step(Z, lo=np.full(n, -1.0), **kw)
    assert "structure-only" not in str(e.value) and "dto_preconditioned_newton_step" in str(e.value)
    with pytest.raises(dto_amd.EngineError, match=word):
        ev.preconditioned_newton_step_dev(8, 1.0, 0, 0, 0, 0, 0, kw.get("radius", 0.0), kw.get("shift", 0.0), kw.get("rtol", 1e-6), kw.get("atol", 0.0),
                                          kw.get("max_iter", 5), False, 8 + 8 * n, 8 + 16 * n)


def test_a_bad_penalty_is_refused_naming_the_row(structure_only):
    ev = structure_only
    n, m = ev.n_variables, ev.n_constraints
    rho = np.full(m, 1.0)
    rho[m - 1] = -2.0
    with pytest.raises(dto_amd.EngineError, match=rf"dto_preconditioned_newton_step: rho\[{m - 1}\]") as e:
        ev.preconditioned_newton_step(np.zeros(n), 1.0, np.zeros(m), rho)
    assert "structure-only" not in str(e.value)


def _call(ev, Z, p, info, mask=None, lo=None, hi=None, trace=None, es=None, zp=None):
    dp = lambda a: None if a is None else a.ctypes.data_as(dto_amd.capi.c_double_p)
    rc = ev._lib.dto_preconditioned_newton_step(ev._h, dp(Z), 1.0, None, None, dp(mask), dp(lo), dp(hi), 0.0, 0.0, 1e-6, 0.0, 5, 0, dp(p), dp(info),
                                                dp(trace), dp(es), dp(zp))
    return rc, ev._lib.dto_last_error(ev._h).decode()


def test_null_pointers_and_overlapping_outputs_are_refused_with_text(structure_only):
    ev = structure_only
    n = ev.n_variables
    Z, p, info = np.zeros(n), np.full(n, np.nan), np.full(16, np.nan)
    for z_, p_, i_ in ((None, p, info), (Z, None, info), (Z, p, None)):
        rc, text = _call(ev, z_, p_, i_)
        assert rc != 0 and "NULL" in text and "dto_preconditioned_newton_step" in text
    assert np.isnan(p).all() and np.isnan(info).all()
    pool = np.zeros(8 * n)
    part = lambda k: pool[k * n:(k + 1) * n]
    Z, mask, lo, hi, p, es, zp = (part(k) for k in range(7))
    for out_name in ("p", "Zp", "entry_state"):
        for k, in_name in enumerate(("Z", "free_mask", "lo", "hi")):
            for alias in (part(k), pool[k * n + n - 1:][:n]):       # the whole vector, and its last entry alone
                outs = dict(p=p, Zp=zp, entry_state=es)
                outs[out_name] = alias
                rc, text = _call(ev, Z, outs["p"], info, mask=mask, lo=lo, hi=hi, es=outs["entry_state"], zp=outs["Zp"])
                assert rc != 0 and f"{out_name} overlaps {in_name}" in text, (out_name, in_name, text)
                assert "structure-only" not in text
    rc, text = _call(ev, Z, p, info, mask=mask, lo=lo, hi=hi, es=es, zp=zp)
    assert rc != 0 and "structure-only" in text, "disjoint buffers: the handle is judged next"
    assert np.isnan(info).all() and not pool.any(), "nothing was written"
    # dto_newton_precondition: z against r and the mask, n_cols, NULL
    dp = lambda a: None if a is None else a.ctypes.data_as(dto_amd.capi.c_double_p)
    buf = np.zeros(5 * n)
    call = lambda mask_, cols, r_, z_: (ev._lib.dto_newton_precondition(ev._h, dp(mask_), cols, dp(r_), dp(z_)), ev._lib.dto_last_error(ev._h).decode())
    rc, text = call(None, 2, buf[:2 * n], buf[2 * n - 1:4 * n - 1])
    assert rc != 0 and "z overlaps r" in text
    rc, text = call(buf[4 * n:], 2, buf[:2 * n], buf[2 * n + 1:4 * n + 1])
    assert rc != 0 and "z overlaps free_mask" in text
    for cols in (0, -2):
        rc, text = call(None, cols, buf[:n], buf[n:2 * n])
        assert rc != 0 and "n_cols" in text
    for r_, z_ in ((None, buf[:n]), (buf[:n], None)):
        rc, text = call(None, 1, r_, z_)
        assert rc != 0 and "NULL" in text
    rc, text = call(buf[4 * n:], 2, buf[:2 * n], buf[2 * n:4 * n])
    assert rc != 0 and "structure-only" in text and not buf.any()
    assert ev._lib.dto_newton_precondition_dev(ev._h, None, 1, 1 << 20, (1 << 20) + 8 * (n - 1), None) != 0
    assert "z overlaps r" in ev._lib.dto_last_error(ev._h).decode()
    assert ev.jacobian_structure()[0].size == ev.n_jacobian_entries


def test_the_docstrings_exist():
    E = dto_amd.Evaluator
    for f in (E.preconditioned_newton_step, E.preconditioned_newton_step_dev, E.newton_pairs_push, E.newton_pairs_info, E.newton_precondition,
              E.newton_precondition_dev, E.newton_pairs_push_dev, E.newton_pairs_clear):
        assert f.__doc__ and len(f.__doc__) > 60, f.__name__
