"""CPU checks of the GEMM descriptor reference (tests/gemm_desc_ref.py) on every descriptor the GPU tests use: the derived
bound is one a correct fp64 evaluation meets, the poison masks agree with a per-element statement of the tri flags and K
bounds, and the size formulas agree with the generator's own layout."""
import numpy as np
import pytest

from tests import gemm_desc_ref as R
from tests import test_gpu_gemm_desc as G

from dataclasses import replace


def _descriptors():
    """(id, descriptor, tile) of EVERY descriptor the GPU tests launch: each GPU test registers the function it takes its
    descriptors from (G.CASES), and its own parametrize marks give the parameters."""
    out = []
    for name, fn, test in G.CASES:
        for n, ps in enumerate(G.param_sets(test)):
            for i, (d, fam) in enumerate(fn(**ps)):
                out.append((f"{name}-{n}-{i}", d, R.FAM_TILE[fam & 255]))
    return out


def _unique(cases, key):
    seen = {}
    for c in cases:
        seen.setdefault(key(c), c)
    return list(seen.values())


ALL = _descriptors()
# each check runs once per distinct input of what it checks
# the masks: shape, layouts of the operands, flags, bounds, tail form and the tile (not batch, strides, alpha / beta)
MASKS = _unique(ALL, lambda c: (c[1].M, c[1].N, c[1].K, c[1].transA, c[1].b_n, c[1].tri, c[1].lower_only, c[1].kb_m, c[1].kb_n, c[1].ke_n,
                                c[1].tail, c[1].dout, c[2]))
# the bound: the values of one problem (not layout, batch or tile)
BOUNDS = _unique(ALL, lambda c: (c[1].M, c[1].N, c[1].K, c[1].tri, c[1].lower_only and c[1].M == c[1].N, c[1].kb_m, c[1].kb_n, c[1].ke_n,
                                 c[1].alpha, c[1].beta, c[1].tbeta, c[1].has_D, c[1].tail, c[1].has_tD))
# the sizes: the whole layout (not alpha / beta)
SIZES = _unique(ALL, lambda c: replace(c[1], alpha=1.0, beta=0.0, tbeta=0.0))


def _ids(cases):
    return [c[0] for c in cases]


def test_every_gpu_test_registers_its_descriptors():
    """A GPU test that launches a product takes its descriptors from a registered function (the refusal tests launch none)."""
    registered = {name for name, _, _ in G.CASES}
    tests = {n for n in dir(G) if n.startswith("test_")}
    assert tests - registered == {"test_direct_output_refusals", "test_refusals"}
    assert len(ALL) > 500 and all(c[1].batch % c[1].nb1 == 0 for c in ALL)


def test_longdouble_is_wider_than_double():
    """The (K + 4) factor rests on a reference with eps <= 2^-63; otherwise the module says so and uses (2 K + 4)."""
    if np.finfo(np.longdouble).eps <= 2.0 ** -63:
        assert R.LONGDOUBLE_OK and R.tol_factor(100) == 104
    else:
        assert not R.LONGDOUBLE_OK and R.tol_factor(100) == 204


@pytest.mark.parametrize("case", BOUNDS, ids=_ids(BOUNDS))
def test_float64_matmul_meets_the_bound(case):
    """NumPy's own float64 evaluation of the operation on the module's operands stays within the bound."""
    _, d, tile = case
    d = R.pick(d, R.logical(d, 11), d.batch - 1)[0] if d.batch > 2 else d
    data = R.logical(d, 11)
    refs = R.reference(d, data)
    za, zb = R.zero_masks(d)
    for z in range(d.batch):
        zp = z // d.nb1
        a = np.where(za, 0.0, data["A"][z][:d.M])
        b = np.where(zb, 0.0, data["B"][z])
        addend = data["D"][zp] if d.has_D else data["C"][z]
        got = d.alpha * (a @ b)
        if d.beta != 0.0:
            got = got + d.beta * addend[:d.M]
        assert R.within(got, refs[z]["ref"], refs[z]["mag"], d.K)
        assert R.worst(got, refs[z]["ref"], refs[z]["mag"], d.K) > 0.0           # (and the bound is not met by being vacuous)
        if d.tail:
            ta = data["A"][z][d.M] if d.tail == 1 else data["tA"][zp]
            tb = d.beta if d.tail == 1 else d.tbeta
            td = addend[d.M] if d.tail == 1 else (data["tD"][zp] if d.has_tD else data["tC"][zp])
            t = np.zeros(d.N)
            for bn in range(d.N // 64):
                kb, ke = R.tile_range(d, 64, 64, R.tail_owner(d, bn), bn)
                t[bn * 64:bn * 64 + 64] = d.alpha * (ta[kb:ke] @ b[kb:ke, bn * 64:bn * 64 + 64])
            if tb != 0.0:
                t = t + tb * td
            assert R.within(t, refs[z]["tref"], refs[z]["tmag"], d.K)


def test_the_bound_refuses_a_wrong_product():
    """One element off by a few ulps of ITS magnitude sum, a dropped k term, a NaN: all outside the bound."""
    d = R.make(64, 64, 48, "tight")
    data = R.logical(d, 12)
    r = R.reference(d, data)[0]
    good = data["A"][0][:64] @ data["B"][0]
    assert R.within(good, r["ref"], r["mag"], d.K)
    bad = good.copy(); bad[3, 5] += 2 * (d.K + 4) * R.U * r["mag"][3, 5]
    assert not R.within(bad, r["ref"], r["mag"], d.K)
    bad = good.copy(); bad[7, 9] -= data["A"][0][7, 47] * data["B"][0][47, 9]
    assert not R.within(bad, r["ref"], r["mag"], d.K)
    bad = good.copy(); bad[0, 0] = np.nan
    assert not R.within(bad, r["ref"], r["mag"], d.K)


@pytest.mark.parametrize("case", MASKS, ids=_ids(MASKS))
def test_poison_masks_agree_with_brute_force(case):
    """Per element (m, n) the terms k in [lo, hi) are not declared zero.  A tile's K range is the hull of its elements' ranges,
    [min lo, max hi) (empty when that is); what no tile reads is poison, everything else is not; and what is read but declared
    zero holds a real zero."""
    _, d, tile = case
    BM, BN = tile
    assert not (d.lower_only and BN > BM)            # (the 64 x 128 tile takes no lower-only launch)
    lo, hi = R.elem_bounds(d)
    ra = np.zeros((d.M, d.K), bool)
    rb = np.zeros((d.K, d.N), bool)
    for bm in range(d.M // BM):
        for bn in range(d.N // BN):
            rs, cs = slice(bm * BM, (bm + 1) * BM), slice(bn * BN, (bn + 1) * BN)
            # lower_only: a tile is worked on when some element of it lies on or below the diagonal of tiles of its own width
            if d.lower_only and not ((np.arange(d.N)[None, cs] // BN) * BN <= np.arange(d.M)[rs, None]).any():
                continue
            kb, ke = int(lo[rs, cs].min()), int(hi[rs, cs].max())
            assert (kb, max(ke, kb)) == R.tile_range(d, BM, BN, bm, bn), (bm, bn)
            ra[rs, kb:ke] = True
            rb[kb:ke, cs] = True
    ma, mb, mt = R.read_masks(d, tile)
    assert np.array_equal(ma, ra) and np.array_equal(mb, rb)
    # soundness: every term that is not declared zero, of every element that is written, reads unpoisoned operands
    k = np.arange(d.K)[None, None, :]
    # (written: the tiles with bn <= bm of the kernel's own size, 32 / 64 / 128 wide)
    fam = {(32, 32): R.FAM_LL, (128, 128): R.FAM_BIG}.get(tile, R.FAM_REG32)
    live = (k >= lo[:, :, None]) & (k < hi[:, :, None]) & R.written_mask(d, fam)[:, :, None]
    assert not (live & ~ma[:, None, :]).any()
    assert not (live & ~mb.T[None, :, :]).any()
    # the buffers: NaN exactly where nothing reads, zeros where a read element is declared zero
    data = R.logical(d, 13)
    buf = R.build(d, data, tile)
    ix = R.index_maps(d)
    za, zb = R.zero_masks(d)
    for z in (0, d.batch - 1):
        a = buf["A"][ix["A"][z]][:d.M]
        b = buf["B"][ix["B"][z]]
        assert np.array_equal(np.isnan(a), ~ma) and np.array_equal(np.isnan(b), ~mb)
        assert np.all(a[ma & za] == 0.0) and np.all(b[mb & zb] == 0.0)
        assert np.array_equal(a[ma & ~za], data["A"][z][:d.M][ma & ~za])
    if d.tail:
        t = buf["A"][ix["A"][0]][d.M] if d.tail == 1 else buf["tA"][ix["tA"][0]]
        assert np.array_equal(np.isnan(t), ~mt)


@pytest.mark.parametrize("case", SIZES, ids=_ids(SIZES))
def test_size_formulas_agree_with_the_generator(case):
    """need() -- the furthest element addressed plus one -- against the largest index the generator's layout produces; and no two
    problems' logical elements share a place (outputs), nothing outside them is anything but the sentinel."""
    _, d, tile = case
    sz = R.need(d)
    ix = R.index_maps(d)
    for nm in ("A", "B", "C", "D", "tA", "tC", "tD"):
        if ix[nm]:
            assert max(int(i.max()) for i in ix[nm]) + 1 == sz[nm], nm
            assert min(int(i.min()) for i in ix[nm]) == 0, nm
        else:
            assert nm not in sz
    allc = np.concatenate([i.ravel() for i in ix["C"]])
    assert np.unique(allc).size == allc.size
    buf = R.build(d, R.logical(d, 14), tile)
    for nm in ("A", "B", "C"):
        assert buf[nm].size == sz[nm]
        inside = np.zeros(sz[nm], bool)
        for i in ix[nm]:
            inside[i] = True
        assert (~inside).any(), f"{nm}: no padding to poison"
        if nm == "C":
            assert np.all(buf[nm].view(np.uint64)[~inside] == R.OUT_SENTINEL)
        else:
            assert np.isnan(buf[nm][~inside]).all()
    if d.dout:
        si = ((d.np_ - 1) * d.o_k + d.o_k - 1) * d.o_ld + d.o_j0 + d.o_cols
        assert sz["samples"] == si and sz["mean"] == (d.np_ - 1) * d.o_n + d.o_j0 + d.o_cols
