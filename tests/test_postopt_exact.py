"""CPU checks of tests/_exact_sums.py: the tile constants are read from lpx_postopt.hip as the kernels declare them and the
cases derived from them cross every tile edge; the error-free products are exact; and the exact-sum checker accepts the
restatement tests/_postopt_ref.py at tile-crossing sizes but rejects a term dropped at a tile edge, a term counted twice,
a term read from the wrong row or column, and results swapped between neighbouring rows or columns."""
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _exact_sums as X                       # noqa: E402
import _postopt_ref as P                      # noqa: E402

TILE = X.postopt_tiling()
SEG, NT, CR, CT, RT = (TILE[k] for k in ("SEG", "NT", "CR", "CT", "RT"))


# ---- tiling -----------------------------------------------------------------------------------------------------------
def test_tiling_matches_the_kernel_asserts_and_the_header():
    assert SEG == P.SEG
    assert CT % SEG == 0 and NT == CT                 # static_asserts of lpx_postopt.hip
    assert CR * (CT // SEG) <= NT
    assert RT == 2 * NT                               # two columns per lane in po_row_pass


def test_tiling_follows_an_edit_of_the_source(tmp_path):
    src = open(X.POSTOPT_SRC).read()
    edited = re.sub(r"(PO_CR\s*=\s*)\d+", r"\g<1>16", src)
    edited = re.sub(r"(PO_NT\s*=\s*)\d+", r"\g<1>128", edited)
    edited = re.sub(r"(PO_CT\s*=\s*)\d+", r"\g<1>128", edited)
    assert edited != src
    f = tmp_path / "lpx_postopt.hip"
    f.write_text(edited)
    t = X.postopt_tiling(src=str(f))
    assert (t["CR"], t["NT"], t["CT"], t["RT"]) == (16, 128, 128, 256)
    assert X.col_rows(t)[0] == 15 and X.col_terms(t)[0] == 127
    with pytest.raises(AssertionError):
        bad = tmp_path / "bad.hip"
        bad.write_text(src.replace("PO_NT = ", "PO_NT = sizeof(double) + "))
        X.postopt_tiling(src=str(bad))


def test_derived_cases_cross_every_edge():
    Ks = X.col_terms(TILE)
    for k in (CT - 1, CT, CT + 1, CT + SEG - 1, CT + SEG, CT + SEG + 1, 2 * CT - 1, 2 * CT + 1):
        assert k in Ks
    assert max(Ks) > 3 * CT and max(Ks) % CT not in (0, SEG)          # a ragged fourth term tile
    Rs = X.col_rows(TILE)
    assert min(Rs) < CR < Rs[1] < NT and max(Rs) > 2 * NT and max(Rs) % CR == 1
    shapes = X.row_shapes(TILE)
    assert [C for _, C in shapes] == [NT, NT + 1, RT - 1, RT, RT + 1, 2 * RT - 1, 2 * RT + 1, 3 * RT + 1]
    assert {NT, NT + 1, 2 * NT + 1} <= {R for R, _ in shapes}
    assert all(C > R + 1 for R, C in shapes)
    assert any((C + 1) % 16 == 0 for _, C in shapes) and any(C % 2 for _, C in shapes)
    assert X.row_terms(TILE, 300) == [SEG - 1, SEG, SEG + 1, 2 * SEG + 1, 300]
    e = X.tile_edges(2 * NT + CR + 1, CR, NT)
    assert {0, CR - 1, CR, NT - 1, NT, 2 * NT, 2 * NT + CR} <= set(e) and e[-1] == 2 * NT + CR


# ---- error-free products ----------------------------------------------------------------------------------------------
def test_two_product_is_exact():
    g = np.random.default_rng(1)
    a = g.standard_normal(3000) * 10.0 ** g.integers(-30, 30, 3000)
    b = g.standard_normal(3000) * 10.0 ** g.integers(-30, 30, 3000)
    a[:3] = [1.0 + 2.0 ** -52, -0.0, 3.0]
    b[:3] = [1.0 - 2.0 ** -53, 5.0, 1.0 / 3.0]
    p, e = X.two_product(a, b)
    for x, y, pp, ee in zip(a.tolist(), b.tolist(), p.tolist(), e.tolist()):
        assert Fraction(x) * Fraction(y) == Fraction(pp) + Fraction(ee)


def test_checker_agrees_with_fractions_on_a_sample():
    """The exact sum of the checker (fsum over two-products) is the Fraction sum: an output one ulp inside the bound
    passes, the exact value rounded passes, and a value moved by twice the bound fails."""
    g = np.random.default_rng(2)
    K = 2 * SEG + 3
    T = g.standard_normal((4, K + 1))
    cols = np.arange(K)
    v = g.standard_normal(K)
    base = T[:, -1]
    exact = [Fraction(float(base[i])) + sum(Fraction(float(v[k])) * Fraction(float(T[i, k])) for k in range(K))
             for i in range(4)]
    out = np.array([float(x) for x in exact])
    assert not X.check_col(T, [base], cols, v, out, range(4), SEG)
    bad = X.check_col(T, [base], cols, v, P.col_combination(T, base, cols, v), range(4), SEG)
    assert not bad
    nseg = (K + SEG - 1) // SEG
    mag = [abs(float(base[i])) + float(sum(abs(Fraction(float(v[k])) * Fraction(float(T[i, k]))) for k in range(K)))
           for i in range(4)]
    far = out + 2.0 * X.gamma(SEG + nseg + 1) * np.array(mag)
    assert len(X.check_col(T, [base], cols, v, far, range(4), SEG)) == 4
    assert X.check_col(T, [base], cols, v, np.array([np.nan, np.inf, out[2], out[3]]), range(4), SEG)[1][0] == 1


# ---- the checker against the restatement and planted faults ---------------------------------------------------------
def _col_case(seed=3):
    g = np.random.default_rng(seed)
    R, C = 2 * NT + CR + 1, 2 * NT + CR + 60
    T = g.standard_normal((R, C))
    K = 3 * CT + SEG + 1
    cols = g.integers(0, C - 1, K)
    cols[CT:CT + 40] = cols[:40]                          # the same columns again in the next term tile
    v = g.standard_normal(K)
    return T, cols, v


def test_column_checker_accepts_the_restatement_and_rejects_planted_faults():
    T, cols, v = _col_case()
    R = T.shape[0]
    base = T[:, -1]
    rows = np.arange(R)
    good = P.col_combination(T, base, cols, v)
    assert not X.check_col(T, [base], cols, v, good, rows, SEG)
    # the new column: base +0.0 but for the objective row
    b2 = np.zeros(R)
    b2[-1] = 0.75
    assert not X.check_col(T, [b2], cols, v, P.col_combination(T, b2, cols, v), rows, SEG)
    # a term dropped at a tile edge: the first term of the second term tile
    drop = P.col_combination(T, base, np.delete(cols, CT), np.delete(v, CT))
    assert len(X.check_col(T, [base], cols, v, drop, rows, SEG)) == R
    # a term counted twice: the last term of the first tile again at the start of the second
    dup = P.col_combination(T, base, np.insert(cols, CT, cols[CT - 1]), np.insert(v, CT, v[CT - 1]))
    assert len(X.check_col(T, [base], cols, v, dup, rows, SEG)) == R
    # one term read from the column next to its own
    c2 = cols.copy()
    c2[2 * CT + SEG] = (c2[2 * CT + SEG] + 1) % (T.shape[1] - 1)
    assert len(X.check_col(T, [base], cols, v, P.col_combination(T, base, c2, v), rows, SEG)) == R
    # the results of the rows on either side of a row tile / combine block edge swapped (a wrong slab row)
    for i in (CR - 1, NT - 1, 2 * NT - 1):
        sw = good.copy()
        sw[[i, i + 1]] = sw[[i + 1, i]]
        assert sorted(r for r, *_ in X.check_col(T, [base], cols, v, sw, rows, SEG)) == [i, i + 1]
    # the last segment left out of the combine
    short = P.col_combination(T, base, cols[: len(cols) - 1], v[: len(v) - 1])
    assert len(X.check_col(T, [base], cols, v, short, rows, SEG)) == R


def test_row_checker_accepts_the_restatement_and_rejects_planted_faults():
    g = np.random.default_rng(4)
    R, C = NT + 1, 2 * RT + 1
    m, Cm = R - 1, C - 1
    T = g.standard_normal((R, C))
    basis = g.choice(Cm, size=m, replace=False).astype(np.int32)
    K = 2 * SEG + 1
    rows = g.integers(0, m, K)
    w = g.standard_normal(K)
    nb = np.setdiff1d(np.arange(Cm), basis)
    dcols = nb[:5]
    dd = g.standard_normal(5)
    Tw, _ = P.objective_update(T, basis, rows, w, dcols, dd)
    d = np.zeros(C)
    d[dcols] = -dd
    cols = np.r_[nb, Cm]
    assert not X.check_row(T, [T[m], d], rows, w, Tw[m], cols, SEG)
    assert X.plus_zero(Tw[m, basis])
    # a term dropped at a segment edge
    Td, _ = P.objective_update(T, basis, np.delete(rows, SEG), np.delete(w, SEG), dcols, dd)
    assert len(X.check_row(T, [T[m], d], rows, w, Td[m], cols, SEG)) == len(cols)
    # a term counted twice
    Tt, _ = P.objective_update(T, basis, np.insert(rows, SEG, rows[SEG - 1]), np.insert(w, SEG, w[SEG - 1]), dcols, dd)
    assert len(X.check_row(T, [T[m], d], rows, w, Tt[m], cols, SEG)) == len(cols)
    # one term read from the wrong row
    r2 = rows.copy()
    r2[2 * SEG] = (r2[2 * SEG] + 1) % m
    Tr, _ = P.objective_update(T, basis, r2, w, dcols, dd)
    assert len(X.check_row(T, [T[m], d], rows, w, Tr[m], cols, SEG)) == len(cols)
    # the sparse cost delta forgotten on one column
    Tn, _ = P.objective_update(T, basis, rows, w, dcols[1:], dd[1:])
    assert [j for j, *_ in X.check_row(T, [T[m], d], rows, w, Tn[m], cols, SEG)] == [dcols[0]]
    # two neighbouring columns across a workgroup edge swapped
    j = RT - 1 if (RT - 1) in nb and RT in nb else int(nb[nb > RT - 1][0])
    sw = Tw[m].copy()
    sw[[j, j + 1]] = sw[[j + 1, j]]
    flagged = [c for c, *_ in X.check_row(T, [T[m], d], rows, w, sw, cols, SEG)]
    assert j in flagged


def test_row_checker_on_the_new_row():
    """add_row: output column C reads the old RHS column Cm; reading column Cm - 1 instead is caught."""
    g = np.random.default_rng(5)
    R, C = NT + 1, RT + 1
    m, Cm = R - 1, C - 1
    T = g.standard_normal((R, C))
    basis = g.choice(Cm, size=m, replace=False).astype(np.int32)
    K = m
    rows = g.integers(0, m, K)
    w = g.standard_normal(K)
    base = g.standard_normal(C + 1)
    base[Cm] = 1.0
    Tw, bw = P.add_row(T, basis, rows, w, base)
    nb = np.setdiff1d(np.arange(Cm), basis)
    out_cols = np.r_[nb, C]
    src = np.r_[nb, Cm]
    assert not X.check_row(T, [base], rows, w, Tw[m], out_cols, SEG, src=src)
    assert Tw[m, Cm] == base[Cm] and X.plus_zero(Tw[m, basis]) and X.plus_zero(Tw[:m, Cm])
    src_bad = np.r_[nb, Cm - 1]
    assert [j for j, *_ in X.check_row(T, [base], rows, w, Tw[m], out_cols, SEG, src=src_bad)] == [C]
