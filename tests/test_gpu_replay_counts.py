"""-m gpu: the count replay the PnP and essential-matrix select kernels share (csrc/solver_dev.h ransac_replay_counts) against the
sequential loop it restates, on hand-made rows of counts that put its records and its iteration cap on the chunk edges."""
import numpy as np
import pytest
import torch

from mapfree_reloc_amd import solver_ops as ops
from oracle import oracle_lib as O

pytestmark = pytest.mark.gpu
MAX_ITERS, N, CONF = 200, 100, 0.9999


def _sequential(cnt, mp):
    """RANSACPointSetRegistrator::run over precomputed counts -> (best, bit, iterations run)"""
    best, bit, niters, it = mp - 1, -1, len(cnt), 0
    while it < niters:
        if cnt[it] > best:
            best, bit = int(cnt[it]), it
            niters = O.update_num_iters(CONF, (N - best) / N, mp, niters)
        it += 1
    return best, bit, it


@pytest.mark.parametrize("mp", [4, 5])
def test_replay_counts_matches_sequential_loop(mp):
    c = np.full((6, MAX_ITERS), mp - 1, dtype=np.int32)
    c[0, 63] = 10; c[0, 70] = 12      # a record in lane 63 of the first chunk, carried into the second
    c[1, 64] = 10                     # a record in lane 0 of the second chunk
    c[2, 5] = 90; c[2, 20] = 95       # the cap drops inside the chunk: the later record lies beyond it
    c[3, 50] = N                      # the cap drops to 0, below bit + 1
    c[4] = 0; c[4, ::7] = -1          # no record at all
    # row 5: every count equal to model_points - 1
    want = np.array([_sequential(row, mp) for row in c], dtype=np.int32)
    cap2 = O.update_num_iters(CONF, (N - 90) / N, mp, MAX_ITERS)
    assert 6 < cap2 <= 20                                                       # the rows are what their comments say
    np.testing.assert_array_equal(want[:, :2], [[12, 70], [10, 64], [90, 5], [N, 50], [mp - 1, -1], [mp - 1, -1]])
    np.testing.assert_array_equal(want[:, 2], [MAX_ITERS, MAX_ITERS, cap2, 51, MAX_ITERS, MAX_ITERS])
    got = ops.test_replay_counts(torch.from_numpy(c).to("cuda:0"), N, CONF, mp).cpu().numpy()
    np.testing.assert_array_equal(got, want)
