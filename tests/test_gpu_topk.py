"""The device top-k selection (order_image, topk_images_kernel, topk_hist_kernel / topk_pick_kernel, lds_radix_select, the
sampled threshold, topk_gather_kernel, topk_compact_kernel, finalize_region_kernel's direct image) against an exact sort, at
its edges.

Every case orders one-row groups by a first term drawn from the edge values of the order image and then by the unique `k`,
so the returned k sequence is one fixed sequence: it must equal the reference's (tests/topk_util.py) with no tie allowance.
The candidates the device kept are bounded from below by C_exact — the groups whose first term collates at or before the
keep-th row's: a smaller set has dropped a row that the second term could have ranked first — and, where distinct collation
classes have distinct images, must be exactly that many.  tests/test_topk_reference_cpu.py proves per case that the
reference alone puts keep where the case says it does.

The image must be equal on values the collation ties: family A holds -0.0, 0.0 and INT 0, which tie, with keep inside that
tie class, on its last row and one past it — every tied group has to be a candidate, whichever zero it holds.
"""
import pytest

import parity_util as pu
import topk_util as tk
from oracle import n1o

pytestmark = pytest.mark.gpu

_TABLES = {}


def _table(case):
    """(table, oracle aggregates by k) of a case; shared by the cases that name the same table."""
    hit = _TABLES.get(case.table)
    if hit is None:
        t = tk.build_table(case.pool, case.idx, case.form)
        keys, aggs, _, kpos, _ = tk.query(case.form, "min", False, False)
        both = aggs if case.form == "key" else sorted(["count(*)", "min(%s)" % tk.D("v"), "max(%s)" % tk.D("v")])
        ora = n1o.run(t, None, keys, both, threads=2)
        assert len(ora.keys) == case.n
        hit = _TABLES[case.table] = (t, both, {key[kpos][1]: (key, agg) for key, agg in zip(ora.keys, ora.aggs)})
    return hit


def _run(case, **extra):
    t, ora_aggs, ora = _table(case)
    keys, aggs, order, kpos, tpos = tk.query(case.form, case.agg, case.desc, case.kdesc)
    e = case.expected()
    opts = {**case.options, **extra}
    gpu, stats = pu.run_gpu(t, None, keys, aggs, order=order, limit=case.limit, offset=case.offset, **opts)
    got = [key[kpos][1] for key in gpu.keys]
    assert got == e.ks, ("rows differ from the exact order", opts, "first difference at",
                         next(((i, g, x) for i, (g, x) in enumerate(zip(got + [None], e.ks + [None])) if g != x), None), got[:12], e.ks[:12])
    for key, agg in zip(gpu.keys, gpu.aggs):  # the returned groups' values: the oracle's, and the reference's first term
        okey, oagg = ora[key[kpos][1]]
        assert pu._canon_key(key) == pu._canon_key(okey), (key, okey)
        for name, g in zip(aggs, agg):
            assert tk.same_value(g, oagg[ora_aggs.index(name)]), (key, name, g, oagg)
        term = tk.first_term(case.pool[int(case.idx[key[kpos][1]])], case.form)
        assert tk.same_value(agg[tpos] if tpos is not None else key[0], term), (key, agg, term)
    return e, stats


def _check_candidates(case, e, stats, exact=True):
    ncand = stats["topk_candidates"]
    if case.claim is None:
        assert ncand == 0, "offset + limit outside (0, groups): the filter has nothing to cut"
        return
    assert e.c_exact <= ncand <= case.n and e.keep <= ncand, (ncand, e.c_exact, e.keep, case.n)
    if not case.injective:
        return
    if exact:
        assert ncand == e.c_exact, (ncand, e.c_exact)
    else:
        # the sampled route: topk_refine_kernel leaves exactly the groups at or below the exact threshold; only when more than
        # kTopkSample groups pass the sample's bound (no refine) do all of those stay; a sample that fell short is followed
        # by the exact select
        assert ncand == e.c_exact or ncand > tk.K_TOPK_SAMPLE, (ncand, e.c_exact)


EXACT = tk.exact_cases()


@pytest.mark.parametrize("case", EXACT, ids=[c.id for c in EXACT])
def test_exact_select_returns_the_exact_rows(case):
    """Families A - F and H: 2 560 groups through topk_images_kernel and the eight histogram / pick passes, with the sampled
    threshold switched off and at its default (too few groups to sample: the same route)."""
    for sample in (0, 1):
        e, stats = _run(case, topk_sample=sample)
        _check_candidates(case, e, stats)


@pytest.mark.parametrize("byte", tk.DIGIT_BYTES, ids=["byte%02x" % b for b in tk.DIGIT_BYTES])
@pytest.mark.parametrize("pas", range(8), ids=["pass%d" % p for p in range(8)])
def test_threshold_on_a_lane_seam_of_every_radix_pass(pas, byte):
    """Family G: the keep-th image's byte in pass `pas` sits on an end or a lane seam of topk_pick_kernel's walk (lane l owns
    bins 4l .. 4l + 3), with images of the same prefix on both sides; ASC, and DESC where the byte is the complement."""
    for desc in (False, True):
        case = tk.digit_case(pas, byte, desc)
        e, stats = _run(case, topk_sample=0)
        _check_candidates(case, e, stats)


SAMPLED = tk.sampled_cases()


@pytest.mark.parametrize("case", SAMPLED, ids=[c.id for c in SAMPLED])
def test_sampled_threshold_at_its_size_bounds(case):
    """65 535 groups (exact route), 65 536 (the first size that samples, stride 4), 65 537, 81 919 (the largest with stride 4:
    the last 16 383 slots of the device's group array are never sampled), keep on either side of topk_can_sample's bound, and
    a flood that takes topk_refine_kernel's no-refine branch: with the sample and with the exact select, both equal to the
    reference.  Which groups land in the never-sampled slots is the engine's own (a group's slot follows from its key's hash),
    so the two 81 919 layouts only place the smallest, or the largest, value at k >= 65 536: they do not control the tail."""
    for sample in (1, 0):
        e, stats = _run(case, topk_sample=sample, device_resident=True)
        _check_candidates(case, e, stats, exact=not (sample and tk.can_sample(case.n, case.keep)))


LEAN = tk.lean_cases()


@pytest.mark.parametrize("lean", [1, 0], ids=["direct-image", "every-row"])
@pytest.mark.parametrize("case", LEAN, ids=[c.id for c in LEAN])
def test_lean_route_images_straight_from_the_region(case, lean):
    """agg_mode=4, one batch: the groups stay in the partitioned path's region and finalize_region_kernel writes the order
    image itself (lean_topk=1); with lean_topk=0 the same groups go through topk_images_kernel."""
    e, stats = _run(case, lean_topk=lean)
    assert stats["agg_mode"] == 4
    _check_candidates(case, e, stats)
