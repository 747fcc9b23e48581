"""lanczos_reference.Lap2dOperator, the matrix-free generate_lap2d_matrix of tests/test_gpu_lanczos_tiles.py, against the dense
matrix of oracle.generate_lap2d at sizes where both fit: exactly on integer-valued operands (every product and sum is an integer
below 2^53, any order gives the same bits), and within the suite's summation-order bound (oracle.gemv_rows_outside) on Gaussian
ones.  n = 1000 and 1023 (floor(sqrt(n)) = 31 both, neither a multiple of the row chunks), float64 and longdouble, 1-D and 2-D."""
import numpy as np
import pytest

import lanczos_reference as ref

LD = np.longdouble
_CACHE = {}


def _case(oracle, n):
    if n not in _CACHE:
        A = oracle.generate_lap2d(n)
        A.setflags(write=False)
        _CACHE[n] = (A, A.astype(LD), ref.Lap2dOperator(oracle, n), ref.Lap2dOperator(oracle, n, chunk=333))
    return _CACHE[n]


@pytest.mark.parametrize("n", [1000, 1023])
def test_the_operator_holds_the_dense_matrix(oracle, n):
    A, _, op, op333 = _case(oracle, n)
    assert op.shape == (n, n) and op.nnz == np.count_nonzero(A)
    dense = np.zeros((n, n))
    np.add.at(dense, (np.repeat(np.arange(n), op.cols.shape[1]), op.cols.ravel()), op.vals.ravel())
    assert np.array_equal(dense, A)
    assert np.array_equal(op.cols, op333.cols) and np.array_equal(op.vals, op333.vals)   # the row chunks leave no trace
    assert ref.is_operator(op) and ref.as_matrix(op, LD) is op and ref.as_matrix(A, np.float64) is A
    with pytest.raises(TypeError):
        np.ones(n) @ op


@pytest.mark.parametrize("dtype", [np.float64, LD])
@pytest.mark.parametrize("n", [1000, 1023])
def test_integer_operands_bit_for_bit(oracle, n, dtype):
    A, Al, op, op333 = _case(oracle, n)
    M = A if dtype is np.float64 else Al
    rng = np.random.default_rng(n)
    for shape in ((n,), (n, 1), (n, 7)):
        v = rng.integers(-1000, 1001, shape).astype(dtype)
        want = M @ v
        assert want.dtype == dtype and np.any(want != 0)
        for o in (op, op333):
            got = o @ v
            assert got.dtype == dtype and got.shape == want.shape
            if dtype is np.float64:
                assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), shape
            else:                                                 # (a longdouble carries pad bytes: compare the values, and the zeros' signs)
                assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want)), shape
    assert (op @ rng.integers(-5, 6, n)).dtype == np.float64      # anything but longdouble is taken as float64


@pytest.mark.parametrize("dtype", [np.float64, LD])
@pytest.mark.parametrize("n", [1000, 1023])
def test_gaussian_operands_within_the_summation_order_bound(oracle, n, dtype):
    A, Al, op, op333 = _case(oracle, n)
    V = np.random.default_rng(7 * n).standard_normal((n, 3))
    y_ref = Al @ V.astype(LD)                                     # near-exact: 64-bit mantissa, at most 5 terms per row
    abs_ap = np.abs(A) @ np.abs(V)
    Y = op @ V.astype(dtype)
    assert Y.dtype == dtype and np.array_equal(Y, op333 @ V.astype(dtype))
    for j in range(3):
        y = op @ V[:, j].astype(dtype)
        assert np.array_equal(y, Y[:, j])                         # a column of a 2-D operand is the 1-D product
        outside = oracle.gemv_rows_outside(y, y_ref[:, j], abs_ap[:, j], n)
        err = float(np.max(np.abs(y.astype(LD) - y_ref[:, j]) / abs_ap[:, j]))
        print("n=%d %s column %d: max |y - y_ref| / (|A||v|) = %.3e (bound %.3e)" % (n, np.dtype(dtype).name, j, err, 4e-16 * np.sqrt(n)))
        assert len(outside) == 0, (n, j, outside[:8])
        assert np.all(np.isfinite(y)) and float(np.linalg.norm(y.astype(np.float64))) > 0.0
