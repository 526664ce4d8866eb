"""Oracle problems for the TimeDependentBilinearIntegrator over what the device kernels branch on and `O.make_tdb_problem` keeps
fixed (NumPy only): the number of drives (0..7), an explicit modulation list, and where state, controls, time and timestep sit in a
knot.  Data scales are those of `O.make_tdb_problem`: dt in 0.25..0.35, u about 0.4, t = 0.3, 0.6, ..., generators over sqrt(n / 4).

Layouts (components of a knot in order; `f3` / `f1` are filler components nothing reads):

    default      x, u, t, dt
    u_first      u, x, t, dt                 controls below the state
    dt_before_t  dt, t, x, u                 timestep and time first, in that order
    gap          x, f3, u, t, f1, dt         something between every two
    t_is_dt      x, u, dt                    the time variable names the timestep: two parameters of theta share one entry

`with_derivative` puts du[m] right behind u and adds a DerivativeIntegrator(u, du).  Reference values come from
tests/tdb_large_cases.reference, which is general in the offsets; tests/test_tdb_layout_reference.py pins it to `O.OracleEvaluator`
on these problems."""
import numpy as np

import dto_oracle as O
import tdb_block_cases as B

LAYOUTS = {"default": ("x", "u", "t", "dt"),
           "u_first": ("u", "x", "t", "dt"),
           "dt_before_t": ("dt", "t", "x", "u"),
           "gap": ("x", "f3", "u", "t", "f1", "dt"),
           "t_is_dt": ("x", "u", "dt")}

# the four-term mixed list of the GPU tests: begins with a sin, repeats both kinds, a constant term (omega = 0), a negative omega.
# OMEGA_FAST: chosen in tests/test_tdb_layout_reference.py (the largest carrier at which the two references agree within a tenth of
# the GPU bars)
OMEGA_FAST = 2.0
MIXED = (("sin", OMEGA_FAST), ("sin", 0.6), ("cos", 0.0), ("cos", -1.7))
PLAIN = (("cos", 1.7), ("sin", 0.6))   # make_tdb_problem's list


def mods_of_length(n_mod):
    """`n_mod` terms: MIXED, cycled with the fast carrier slowed down each round (omega stays distinct per term)."""
    out = []
    for c in range(n_mod):
        kind, w = MIXED[c % 4]
        out.append((kind, w / (1 + c // 4) if w == OMEGA_FAST else w + 0.37 * (c // 4)))
    return tuple(out)


def place(layout, n, m, with_derivative=False):
    """(offsets by name, z) of a layout; `t` maps to the timestep's entry in "t_is_dt"."""
    off, pos = {}, 0
    for name in LAYOUTS[layout]:
        d = {"x": n, "u": m, "t": 1, "dt": 1, "f3": 3, "f1": 1}[name]
        off[name] = pos
        pos += d
        if name == "u" and with_derivative:
            off["du"] = pos
            pos += m
    off.setdefault("t", off["dt"])
    return off, pos


def lay_out(rows, layout, G, mods, m, order, substeps, with_derivative, rng):
    """Problem from the component rows `x, u, t, dt` (and `du`); filler rows are drawn from `rng`."""
    n, N = rows["x"].shape
    off, z = place(layout, n, m, with_derivative)
    data = np.zeros((z, N))
    names = [c for c in LAYOUTS[layout]] + (["du"] if with_derivative else [])
    for name in names:
        d = {"x": n, "u": m, "du": m, "t": 1, "dt": 1, "f3": 3, "f1": 1}[name]
        data[off[name]:off[name] + d] = rows[name] if name in rows else rng.standard_normal((d, N))
    integ = [O.TimeDependentBilinearIntegrator(off["x"], n, off["u"] if m else 0, m, off["t"], G, list(mods), order,
                                               substeps).bind(z, off["dt"])]
    if with_derivative:
        integ.append(O.DerivativeIntegrator(off["u"], m, off["du"]))
    reg = O.QuadraticRegularizer(off["u"], m, np.ones(m)) if m else O.QuadraticRegularizer(off["x"], n, np.ones(n))
    return O.Problem(N=N, z=z, dt_idx=off["dt"], integrators=integ, objectives=[reg], Z0=data.T.reshape(-1).copy())


def layout_problem(n, m, order, substeps, mods, layout, N=3, seed=None, with_derivative=False):
    """One TimeDependentBilinearIntegrator on random data, bound with the layout's explicit x_off, u_off, t_off, dt_idx, and a
    QuadraticRegularizer on u (on x without drives).  mods: [(kind, omega)]; G and the H arrays are drawn as in make_tdb_problem."""
    if with_derivative and not m:
        raise ValueError("with_derivative needs a drive")
    rng = np.random.default_rng(40 + n if seed is None else seed)
    rows = {"x": rng.standard_normal((n, N)), "u": 0.4 * rng.standard_normal((m, N)),
            "t": np.cumsum(np.full(N, 0.3))[None, :], "dt": 0.25 + 0.1 * rng.random((1, N))}
    s = 1.0 / np.sqrt(n / 4.0)
    G = rng.standard_normal((m + 1, n, n)) * s
    mods = [(kind, float(w), 0.5 * rng.standard_normal((m + 1, n, n)) * s) for kind, w in mods]
    if with_derivative:
        rows["du"] = rng.standard_normal((m, N))
    return lay_out(rows, layout, G, mods, m, order, substeps, with_derivative, rng)


def kron_layout_problem(b, r, m, order, substeps, mods, layout, N=3, with_derivative=False):
    """The twin for replicated blocks: tdb_block_cases' family (every matrix kron(I_r, B)) with the carriers of `mods`, the data of
    tdb_block_cases.problem_from_family, re-laid."""
    rng = np.random.default_rng(1000 * b + r)
    G, drawn = B.kron_family(b, r, m, 0, rng)
    s = 1.0 / np.sqrt(b / 4.0)
    mods = [(kind, float(w), np.stack([np.kron(np.eye(r), Bj) for Bj in 0.5 * s * rng.standard_normal((m + 1, b, b))])) for kind, w in mods]
    base = B.problem_from_family(G, mods, m, order, substeps, N=N, seed=b + r, with_derivative=with_derivative)
    n = b * r
    X = base.Z0.reshape(N, base.z).T
    rows = {"x": X[:n], "u": X[n:n + m], "t": X[base.z - 2:base.z - 1], "dt": X[base.z - 1:]}
    if with_derivative:
        rows["du"] = X[n + m:n + 2 * m]
    return lay_out(rows, layout, G, mods, m, order, substeps, with_derivative, np.random.default_rng(b * r))
