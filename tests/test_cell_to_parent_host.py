"""CPU: h3_cell_to_parent (csrc/k_rollup.h), the roll-up's group-by key, executed on the host through
hm_selftest_cell_to_parent, against upstream cellToParent's rule restated in numpy: the resolution field becomes r,
digits r+1..15 become 7, base cell and digits 1..r stay."""
import numpy as np
import pytest


def parent_rule(c, r):
    c = np.asarray(c, dtype=np.uint64)
    return (c & ~np.uint64(0xF << 52)) | np.uint64(r << 52) | np.uint64((1 << 3 * (15 - r)) - 1)


def cell_to_parent(cells, r):
    import mobheat
    from mobheat._lib import check, ptr
    lib = mobheat.load()
    cells = np.ascontiguousarray(cells, dtype=np.uint64)
    out = np.zeros(cells.size, np.uint64)
    check(lib.hm_selftest_cell_to_parent(ptr(cells), cells.size, int(r), ptr(out)), None, "hm_selftest_cell_to_parent")
    return out


def _res_of(cells):
    return (np.asarray(cells, np.uint64) >> np.uint64(52)) & np.uint64(0xF)


@pytest.fixture(scope="module")
def sphere():
    rng = np.random.default_rng(1207)
    n = 100_000
    return np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, n))), rng.uniform(-180.0, 180.0, n)


@pytest.mark.parametrize("res", range(16))
def test_matches_rule_on_oracle_cells(oracle_h3, sphere, res):
    cells = oracle_h3.latlng_to_cell(sphere[0], sphere[1], res)
    assert cells.size == 100_000 and (_res_of(cells) == res).all()
    for r in range(res + 1):
        got = cell_to_parent(cells, r)
        np.testing.assert_array_equal(got, parent_rule(cells, r), err_msg=f"res {res} -> {r}")
        assert (_res_of(got) == r).all()
    # r == res is the identity
    np.testing.assert_array_equal(cell_to_parent(cells, res), cells)


def test_known_chain():
    c9, c8, c7 = 0x8928308280fffff, 0x8828308281fffff, 0x872830828ffffff
    assert cell_to_parent([c9], 8)[0] == c8
    assert cell_to_parent([c8], 7)[0] == c7
    assert cell_to_parent([c9], 7)[0] == c7
    assert cell_to_parent([c9], 9)[0] == c9


def test_pentagons_and_edge_points(oracle_h3):
    """Cells at the poles, the antimeridian and the other edge points, and the twelve pentagons' own descendants (the
    centre child of a pentagon is a pentagon: the cell at a res-0 pentagon's centre, at every resolution)."""
    from mobheat import synth
    el, eo = synth.edge_points()
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(el) & np.isfinite(eo) & (np.abs(el) <= 90) & (np.abs(eo) <= 180)
    el, eo = el[ok], eo[ok]
    # the pentagon base cells (upstream's baseCellData: 4, 14, 24, 38, 49, 58, 63, 72, 83, 97, 107, 117)
    pent_bc = [4, 14, 24, 38, 49, 58, 63, 72, 83, 97, 107, 117]
    pents0 = np.array([(1 << 59) | (bc << 45) | ((1 << 45) - 1) for bc in pent_bc], np.uint64)
    pla, plo = oracle_h3.cell_to_latlng(pents0)
    for res in range(16):
        cells = oracle_h3.latlng_to_cell(np.r_[el, pla], np.r_[eo, plo], res)
        pc = cells[el.size:]
        # a pentagon's centre lies in its centre child: digits 1..res all 0, the pentagon's base cell
        np.testing.assert_array_equal((pc >> np.uint64(45)) & np.uint64(0x7F), np.array(pent_bc, np.uint64))
        assert ((pc & np.uint64((1 << 45) - 1)) == np.uint64((1 << 3 * (15 - res)) - 1)).all()
        for r in range(res + 1):
            got = cell_to_parent(cells, r)
            np.testing.assert_array_equal(got, parent_rule(cells, r), err_msg=f"res {res} -> {r}")
        np.testing.assert_array_equal(cell_to_parent(pc, 0), pents0)


@pytest.mark.parametrize("res", [15, 9, 4])
def test_parent_of_parent_is_direct_parent(oracle_h3, sphere, res):
    cells = oracle_h3.latlng_to_cell(sphere[0][:20_000], sphere[1][:20_000], res)
    for mid in range(res + 1):
        via = cell_to_parent(cells, mid)
        for r in range(mid + 1):
            np.testing.assert_array_equal(cell_to_parent(via, r), cell_to_parent(cells, r), err_msg=f"{res}->{mid}->{r}")


def test_bad_arguments():
    import mobheat
    from mobheat._lib import HM_E_INVALID, ptr
    lib = mobheat.load()
    c = np.array([0x8928308280fffff], np.uint64)
    out = np.zeros(1, np.uint64)
    assert lib.hm_selftest_cell_to_parent(ptr(c), 1, 16, ptr(out)) == HM_E_INVALID
    assert lib.hm_selftest_cell_to_parent(ptr(c), 1, -1, ptr(out)) == HM_E_INVALID
    assert lib.hm_selftest_cell_to_parent(None, 0, 3, None) == 0
