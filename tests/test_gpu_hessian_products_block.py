"""GPU: block Hessian-of-Lagrangian products Y = H(Z; sigma, mu) V (dto_eval_hessian_products[_dev], k_hess_spmm of
csrc/dto_hess_product.hip) against the single product of every column, BIT FOR BIT: the block kernel keeps k_hess_spmv's summation order per
column.  The three problems put rows into the 4-, 16- and 64-lane classes; 11 columns are one full tile of 8 and a tail of 3.  The
single product itself is held to the oracle in test_gpu_hessian_product.py."""
import numpy as np
import pytest

import dto_oracle as O
from helpers import to_engine

pytestmark = pytest.mark.gpu

SIGMA = 0.7
PROBLEMS = {"n17": lambda: O.make_scaled_problem(5, 17, 3, seed=17, with_constraint=True),
            "n70": lambda: O.make_scaled_problem(4, 70, 2, seed=70, with_constraint=True),
            "n130": lambda: O.make_scaled_problem(3, 130, 2, seed=2, with_constraint=True)}


def single(ev, Z, v, mu):
    y = np.full(ev.n_variables, np.nan)
    ev.eval_hessian_lagrangian_product(y, Z, v, SIGMA, mu)
    return y


def block(ev, Z, V, mu):
    Y = np.full(V.shape, np.nan)
    ev.eval_hessian_lagrangian_products(Y, Z, V, SIGMA, mu)
    return Y


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_every_column_has_the_bits_of_the_single_product(name):
    import dto_amd
    import torch
    p = PROBLEMS[name]()
    Z = np.ascontiguousarray(p.Z0)
    ref, ev = dto_amd.Evaluator(to_engine(p)), dto_amd.Evaluator(to_engine(p))
    try:
        n = ev.n_variables
        mu = np.random.default_rng(3).standard_normal(ev.n_constraints)
        V = np.random.default_rng(5).standard_normal((11, n))
        want = np.stack([single(ref, Z, v, mu) for v in V])
        assert not np.isnan(want).any()

        Y = block(ev, Z, V, mu)                                   # host form, a first call at a new point
        print(name, "new point: entries that differ", int(np.sum(Y != want)), "largest", float(np.max(np.abs(Y - want))))
        assert np.array_equal(Y, want)
        ev.profile_enable(True)
        ev.profile_reset()
        Y = block(ev, Z, V, mu)                                   # the kept point: the product launch alone
        assert np.array_equal(Y, want)
        assert ev.profile_get("hess_product")[1] == 1, "one launch per block call at the kept point, no gather"
        ms, launches, nbytes = ev.profile_get("hess_product")
        assert nbytes > 16.0 * n * 11, "bytes as executed: the vectors per column"

        dev = torch.device("cuda", 0)
        st = torch.cuda.current_stream(dev).cuda_stream
        dZ, dmu, dV = (torch.from_numpy(np.array(a)).to(dev) for a in (Z, mu, V))
        dY = torch.full((11, n), float("nan"), dtype=torch.float64, device=dev)
        ev.profile_reset()
        ev.eval_hessian_products_dev(dZ.data_ptr(), SIGMA, dmu.data_ptr(), 11, dV.data_ptr(), dY.data_ptr(), stream=st)   # kept: same bits of Z, mu
        torch.cuda.synchronize()
        assert np.array_equal(dY.cpu().numpy(), want)
        assert ev.profile_get("hess_product")[1] == 1
        ev.profile_enable(False)

        Z2 = Z * (1.0 + 0.01 * np.random.default_rng(9).standard_normal(Z.size))
        dZ2 = torch.from_numpy(Z2).to(dev)
        dY.fill_(float("nan"))
        ev.eval_hessian_products_dev(dZ2.data_ptr(), SIGMA, dmu.data_ptr(), 11, dV.data_ptr(), dY.data_ptr(), stream=st)  # device form at a new point
        torch.cuda.synchronize()
        want2 = np.stack([single(ref, Z2, v, mu) for v in V])
        assert not np.array_equal(want2, want)
        assert np.array_equal(dY.cpu().numpy(), want2)
        assert np.array_equal(single(ev, Z2, V[4], mu), want2[4]), "a single product at the point the block call kept"

        for width in (1, 3, 64):                                  # chunks of 1, 3 and (one chunk) 11 columns: the same bits
            ev.set_option("reduced_block_width", width)
            assert np.array_equal(block(ev, Z2, V, mu), want2), width
        ev.set_option("reduced_block_width", 0)

        assert np.array_equal(block(ev, Z, V[:1], mu)[0], want[0]), "n_cols = 1 is the single product"
        for k in (2, 4, 5, 8, 9):                                 # the tiles of 2, 4 and 8 columns, full and with a tail
            assert np.array_equal(block(ev, Z, V[:k], mu), want[:k]), k
    finally:
        ev.close()
        ref.close()


def test_refusals():
    import dto_amd
    p = PROBLEMS["n17"]()
    ev = dto_amd.Evaluator(to_engine(p))
    try:
        n = ev.n_variables
        Z, mu = np.ascontiguousarray(p.Z0), np.zeros(ev.n_constraints)
        with pytest.raises(dto_amd.EngineError, match="n_cols = 0"):
            ev.eval_hessian_lagrangian_products(np.zeros((0, n)), Z, np.zeros((0, n)), SIGMA, mu)
        with pytest.raises(dto_amd.EngineError, match="n_cols = 0"):
            ev.eval_hessian_products_dev(1, SIGMA, 1, 0, 1, 1)    # refused before any pointer is read
        with pytest.raises(dto_amd.EngineError, match="NULL"):
            ev.eval_hessian_products_dev(1, SIGMA, 1, 2, 0, 1)
        with pytest.raises(ValueError):
            ev.eval_hessian_lagrangian_products(np.zeros((2, n)), Z, np.zeros((3, n)), SIGMA, mu)   # Y too small for 3 columns
        V = np.random.default_rng(1).standard_normal((2, n))
        assert np.array_equal(block(ev, Z, V, mu)[1], single(ev, Z, V[1], mu)), "the handle stays usable"
    finally:
        ev.close()
