"""The strict-lower mode of a square lower-only product, on paper (tests/sym_skip_ref.py): the masks a launch must write, may
write and must leave alone, and the flops a triangular grid executes with and without staircase bounds, against a brute-force
count.  No GPU."""
import numpy as np
import pytest

from tests import sym_skip_ref as S

SIZES = (64, 128, 192, 768)


@pytest.mark.parametrize("b_n", [0, 1], ids=["B_nk", "B_kn"])
@pytest.mark.parametrize("M", SIZES)
def test_masks_partition_the_block(M, b_n):
    must, may, skip = S.must_write(M), S.may_write(M), S.skipped(M, b_n)
    nt = M // 64
    # what must be written may be written, and is never skipped or above the block diagonal
    assert not (must & ~may).any()
    assert not (must & S.unchanged(M, True, b_n)).any() and not (must & S.unchanged(M, False)).any()
    # what is skipped: six 16 x 16 blocks ([n][k]) or one 32 x 32 quadrant ([k][n]) per diagonal tile, strictly above the element
    # diagonal, inside what may be written
    r, c = np.nonzero(skip)
    per_tile = 32 * 32 if b_n else 6 * 16 * 16
    assert skip.sum() == per_tile * nt and (r < c).all() and not (skip & ~may).any()
    assert skip.sum() == round((1.0 - S.diag_share(b_n)) * 64 * 64) * nt
    # the quadrant is four of the six blocks
    assert not (S.skipped(M, 1) & ~S.skipped(M, 0)).any()
    # may-write = must-write + the strict upper triangles of the diagonal tiles
    upper_of_diag = may & ~must
    rr, cc = np.nonzero(upper_of_diag)
    assert (rr // 64 == cc // 64).all() and (rr < cc).all() and upper_of_diag.sum() == nt * (64 * 63 // 2)
    # the three classes of the 64 x 64 LDS-DMA family cover the block exactly once
    rest = may & ~must & ~skip                                 # written, not needed: the rest of a diagonal tile's upper triangle
    total = must.astype(int) + rest.astype(int) + S.unchanged(M, True, b_n).astype(int)
    assert (total == 1).all()
    # a kernel that does not know the bit leaves only the tiles above the block diagonal
    assert S.unchanged(M, False).sum() == 64 * 64 * nt * (nt - 1) // 2
    assert (S.unchanged(M, True, b_n) & ~S.unchanged(M, False) == skip).all()


def _g2_staircase(nt):
    return tuple(64 * t for t in range(nt))                    # K(bm) = K - 64 bm: the coupling window's steps


@pytest.mark.parametrize("b_n", [0, 1], ids=["B_nk", "B_kn"])
@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("M,K,kb", [(64, 16, None), (128, 64, None), (192, 256, None), (192, 256, (0, 64, 128)), (256, 256, _g2_staircase(4)),
                                    (128, 128, (64, 0))], ids=["64", "128", "192", "192_stairs", "256_stairs", "128_not_monotone"])
def test_executed_flops_against_a_brute_force_count(M, K, kb, strict, b_n):
    assert S.executed_flops(M, K, kb, strict, b_n) == S.executed_flops_brute(M, K, kb, strict, b_n)


def test_the_launches_of_the_batched_factor():
    """The shares the change was planned with (darcy256, blocks of 1024 with a coupling window of 768): G2 runs 364 tile-K units
    of which 78 in diagonal tiles; the rank-256 updates 78 / 36 / 10 tiles of which 12 / 8 / 4 are diagonal.  B is stored [n][k]
    in all of them: a diagonal tile runs 10 of its 16 MFMA blocks."""
    every, diag = S.k_units(768, 768, _g2_staircase(12))
    assert (every, diag) == (364, 78)
    assert S.executed_flops(768, 768, _g2_staircase(12), True) == 2.0 * 64 ** 3 * (364 - 78 * 6 / 16)
    for M, tiles, dtiles in ((768, 78, 12), (512, 36, 8), (256, 10, 4)):
        every, diag = S.k_units(M, 256)
        assert (every, diag) == (4 * tiles, 4 * dtiles)
        assert S.executed_flops(M, 256, None, True) == 2.0 * 64 ** 3 * 4 * (tiles - dtiles * 6 / 16)
    # the 128^2 S_BB update: three tiles, two diagonal
    assert S.k_units(128, 128) == (6, 4)
    assert S.executed_flops(128, 128, None, True) / S.executed_flops(128, 128, None, False) == (6 - 4 * 6 / 16) / 6
