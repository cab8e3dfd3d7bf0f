"""
GPU test of the ORDER of the strided-tree reduction (csrc/rsf_host.h: sum_strided_tree; csrc/rsf_kernel_common.h: wave_sum,
block_fields_store), pinned through the public rsf_pool_joint_partials: "every sum has a fixed order" as a tested statement.

With d = 1, the centre 0.0 and draws that are float32 values widened to float64, x - c is x and x * x is exact in float64, so the
kernel's fused multiply-add equals a multiply and an add and its three sums (count, sum x, sum x^2) are plain float64
additions.  NumPy repeats them in the documented sequence:
    1. per thread, rows g, g + T, g + 2 T, ... in that order from 0.0; T = 256 * blocks, blocks = min(1024, ceil(n / 256));
    2. per wave the shuffle tree off = 32, 16, ..., 1 (lane l adds lane l + off), read at lane 0;
    3. the four waves of a workgroup in index order;
    4. the combine: thread t of 256 adds the workgroups' partials t, t + 256, ... in that order from 0.0;
    5. its shuffle tree and its four waves in index order;
and the result must be EQUAL, bit for bit.  (A thread with no row, or no partial, holds 0.0; adding 0.0 changes no bit of a sum
that started from +0.0, which is how the emulation treats the ragged ends.)

Sizes, the smallest at which each stage can go wrong: 1; 70 (a partial second wave, idle waves add 0.0); 256 * 3 + 5 (fewer
workgroups than lanes in the combine); 256 * 257 + 19 (the combine's stride loop takes a second term in threads 0 and 1);
2 * 256 * 1024 + 77 (the grid is capped, several rows per thread).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BLOCK, WAVE, MAX_BLOCKS = 256, 64, 1024
SIZES = [1, 70, 256 * 3 + 5, 256 * 257 + 19, 2 * 256 * 1024 + 77]


def _strided(v, stride):
    """Thread t of `stride`: 0.0 + v[t] + v[t + stride] + ... in that order; v (fields, len) -> (fields, stride)."""
    rows = -(-v.shape[1] // stride)
    padded = np.zeros((v.shape[0], rows * stride))
    padded[:, : v.shape[1]] = v
    acc = np.zeros((v.shape[0], stride))
    for r in range(rows):
        acc = acc + padded[:, r * stride : (r + 1) * stride]
    return acc


def _workgroup(v):
    """Per workgroup of 256 per-thread values (..., 256): the shuffle tree of each wave at lane 0, then the waves in order."""
    w = v.reshape(v.shape[:-1] + (BLOCK // WAVE, WAVE)).copy()
    off = WAVE // 2
    while off:
        w[..., :off] = w[..., :off] + w[..., off : 2 * off]
        off //= 2
    s = w[..., 0, 0]
    for k in range(1, BLOCK // WAVE):
        s = s + w[..., k, 0]
    return s


def _emulate(x):
    n = x.size
    blocks = min(MAX_BLOCKS, -(-n // BLOCK))
    terms = np.stack([np.ones(n), x, x * x])                       # count, x - 0.0, fma(x, x, .) with x * x exact
    per_thread = _strided(terms, blocks * BLOCK)                   # 1
    part = _workgroup(per_thread.reshape(3, blocks, BLOCK))        # 2, 3: part[field][block]
    return _workgroup(_strided(part, BLOCK))                       # 4, 5


@pytest.fixture(scope="module")
def dev_engine(pkg):
    e = pkg.Engine(mem="device")
    yield e
    e.close()


@pytest.mark.parametrize("n", SIZES)
def test_strided_tree_order(gpu_engine, dev_engine, n):
    import torch

    x = np.random.default_rng(9100 + n).standard_normal(n).astype(np.float32).astype(np.float64)
    assert np.array_equal((x * x).astype(np.longdouble), x.astype(np.longdouble) ** 2)  # the squares are exact
    want = _emulate(x)
    assert want[0] == n
    for name, got in (("host", gpu_engine.pool_joint_partials(x.reshape(n, 1), [0.0])),
                      ("device", dev_engine.pool_joint_partials(torch.as_tensor(x.reshape(n, 1), device="cuda"), [0.0]))):
        print(f"n={n} {name}: got {got[[0, 2, 3]]!r} want {want!r}")
        assert got.shape == (4,) and got[1] == 0.0  # no row left out
        np.testing.assert_array_equal(got[[0, 2, 3]], want, err_msg=f"n={n}, {name} memory")
