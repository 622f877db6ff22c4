"""CPU (`-m "not gpu"`): ties tests/_rowpass_reference.py down before tests/test_gpu_rowpass_entries.py holds the row pass
(k_rowpass, telescope_amd/csrc/tsem_report.hip) against it.

* the reference's own fp64 operator sequence (`numpy_z`, from the oracle) is within bound(len) = (len + 3) 2^-53 of `exact_z`
  (long double), and on rows that are `clear` the exact assignment equals the oracle's, all six methods;
* a numpy emulation of the device's order of additions meets the same bound with room (so a correct kernel has room too);
* `bam_out.tag_word` is numpy's scalar expressions on every planted threshold value;
* the planted rows give z == x bit for bit; the inputs of the GPU legs are clear on >= 99 % of their rows (near-tie matrices: on
  fewer than half).

Each test prints the figures it asserts on (`pytest -s`)."""
import numpy as np
import pytest
import scipy.sparse as sp

import _rowpass_reference as R

LD = R.LD


def _check_assignment(ref, name):
    """exact_assigned == oracle.reassign(method) > 0 on clear rows; `average` / `conf` values within 2 bound(len) of the exact ones"""
    rid = R.row_ids(ref.indptr)
    for m in R.METHODS:
        o, e, clear = ref.assigned(m)
        c = clear[rid]
        bad = np.flatnonzero(((o > 0) != (e > 0)) & c)
        assert len(bad) == 0, (name, m, rid[bad[:5]])
        if m in ('average', 'conf'):
            lim = 2 * R.bound(ref.lens)[rid] * e
            assert np.all((np.abs(o.astype(LD) - e) <= lim) | ~c), (name, m)
        else:
            assert np.array_equal(o[c], e[c].astype(np.float64)), (name, m)


CASES = [('emulation', 400), ('emulation', 5000), ('mixed', 400), ('mixed', 5000), ('single_first_last', 400), ('last_row_longest', 400)]


@pytest.mark.parametrize('which', [R.CUR, R.INITIAL])
@pytest.mark.parametrize('name,max_score', CASES)
def test_numpy_z_is_within_the_bound_of_exact_z(name, max_score, which):
    """random matrices, row lengths 1 - 5000, scores up to 400 and up to 5000"""
    raw, lut, pi, theta = R.emulation_matrix(max_score) if name == 'emulation' else R.shape_case(name, max_score)
    ref = R.Reference(raw, lut, pi, theta, which=which)
    frac = ref.numpy_fraction()
    print('numpy_z %s/%d/%s: %.3f of bound(len), %.2f %% of %d rows clear, %d rows with several best hits'
          % (name, max_score, which, frac, 100 * ref.clear_share(), raw.shape[0], int((ref.nb > 1).sum())))
    assert frac <= 1.0
    assert np.array_equal(ref.zn != 0, ref.inpat & (ref.z != 0))
    assert ref.clear_share() >= 0.99
    _check_assignment(ref, (name, max_score, which))


def test_user_z_is_taken_as_it_is():
    raw, lut, pi, theta = R.shape_case('mixed')
    uz = R.user_z_of(raw, lut, pi, theta)
    ref = R.Reference(raw, lut, which=R.USER, user_z=uz)
    assert np.array_equal(ref.zn, np.where(np.isnan(uz), 0.0, uz)) and ref.numpy_fraction() == 0.0
    _check_assignment(ref, 'user')


def test_device_order_of_additions_meets_the_bound():
    """16 lane-strided partial sums, then a tree over the lanes: 20 000 rows of 1 - 79 entries plus 200 rows of 100 - 4999,
    score_lut(400), Dirichlet parameters.  A correct kernel has room under the bound, and the bound is not slack by orders of
    magnitude."""
    raw, lut, pi, theta = R.emulation_matrix(400)
    ip = raw.indptr.astype(np.int64)
    z, inpat = R.exact_z(ip, raw.indices, raw.data, lut, pi, theta)
    amb = (np.diff(ip) > 1)[R.row_ids(ip)]
    n64 = lut[raw.data] * np.where(amb, (pi * theta)[raw.indices], pi[raw.indices])
    frac = R.error_fraction(R.device_order_z(ip, n64, inpat), z, inpat, ip)
    _, _, clear, clear_thresh, _ = R.exact_assigned(ip, z, inpat, 0.9, methods=())
    print('device order of additions: %.3f of bound(len); %d of %d rows clear' % (frac, int((clear & clear_thresh).sum()), len(clear)))
    assert 0.1 < frac <= 1.0
    assert np.all(clear & clear_thresh)


def test_tag_word_is_numpys_scalar_expressions_on_every_planted_value():
    from telescope_amd import bam_out
    p = R.planted_values()
    assert len(p) > 1000 and p[0] == 0.0 and p[-1] == 1.0 and np.nextafter(1.0, 0.0) in p and 0.2 in p and 0.9 in p
    for assigned in (0, 1):
        got = bam_out.tag_word(p, np.full(len(p), assigned))
        for P, w in zip(p, got):
            mapq = int(round(-10 * np.log10(1 - P))) if P < 1.0 else 255
            want = mapq | int(round(P * 100)) << 8 | assigned << 16 | int(P >= 0.2) << 17
            assert int(w) == want, (P.hex(), int(w), want)
    # the exact XP ties round half to even
    assert [int(w) >> 8 & 0xff for w in bam_out.tag_word(np.array([0.125, 0.375, 0.625, 0.875]), np.zeros(4))] == [12, 38, 62, 88]


@pytest.mark.parametrize('table_len,part,parts', [(2048, 0, 2), (2048, 1, 2), (8192, 0, 1)])
def test_planted_rows_give_z_equal_to_x_bit_for_bit(table_len, part, parts):
    raw, lut, x = R.planted_case(table_len, part, parts)
    assert len(lut) == table_len and np.all(np.diff(lut) > 0)
    rng = np.random.RandomState(3)
    pi, theta = R.dyadic_parameters(raw.shape[1], rng)
    y = 1.0 - x
    for which in (R.INITIAL, R.CUR):
        ref = R.Reference(raw, lut, pi, theta, which=which)
        assert np.array_equal(ref.zn[0::2], x) and np.array_equal(ref.zn[1::2], y), which
        # (the exact sum x + fl(1 - x) is 1 only to within 2^-54: fp64 rounds it to 1, which is what makes fp64's z equal x)
        assert np.all(np.abs(ref.z[0::2] - x) <= R.U * x) and np.all(np.abs(ref.z[1::2] - y) <= R.U * y), which
    uz = np.stack([x, np.where(np.arange(len(x)) % 5 == 4, np.nan, y)], axis=1).ravel()
    ref = R.Reference(raw, lut, which=R.USER, user_z=uz)
    assert np.array_equal(ref.zn, np.where(np.isnan(uz), 0.0, uz))


def test_the_inputs_of_the_gpu_legs_are_clear_where_they_should_be():
    """>= 99 % of the rows of every non-near-tie matrix are clear (so the exact-arithmetic check covers them), fewer than half of
    the rows of the near-tie matrices are (so that leg tests what it is for)."""
    from telescope_amd.likelihood import score_lut
    for name in sorted(R.SHAPES):
        for max_score in (400, 5000):
            if name == 'rows_300000' and max_score == 5000:
                continue
            raw, lut, pi, theta = R.shape_case(name, max_score)
            for which in (R.CUR, R.INITIAL):
                share = R.Reference(raw, lut, pi, theta, which=which).clear_share()
                print('clear rows %s/%d/%s: %.2f %%' % (name, max_score, which, 100 * share))
                assert share >= 0.99, (name, max_score, which)
    for kind in R.DEAD_KINDS:
        raw, lut, pi, theta = R.dead_column_case(kind)
        ref = R.Reference(raw, lut, pi, theta)
        print('clear rows dead/%s: %.2f %%, numpy_z at %.3f of the bound' % (kind, 100 * ref.clear_share(), ref.numpy_fraction()))
        assert ref.clear_share() >= 0.99 and ref.numpy_fraction() <= 1.0, kind
        _check_assignment(ref, kind)
    for seed, kw in R.NEAR_TIE_CASES:
        raw, pi, theta = R.near_tie_matrix(seed, **kw)
        ref = R.Reference(raw, score_lut(int(raw.data.max())), pi, theta)
        print('clear rows near-tie seed %d: %.2f %%, numpy_z at %.3f of the bound' % (seed, 100 * ref.clear_share(), ref.numpy_fraction()))
        assert ref.clear_share() < 0.5 and ref.numpy_fraction() <= 1.0, seed
        _check_assignment(ref, seed)
        ref2 = R.Reference(raw, ref.lut, pi, theta, thresh=R.z_value_threshold(ref))
        assert np.any(ref2.zn == ref2.thresh) and ref2.clear_share() < 0.5
        _check_assignment(ref2, (seed, 'threshold on a z value'))


def test_dead_column_cases_hold_what_they_are_for():
    raw, lut, pi, theta = R.dead_column_case('pi')
    _, inpat = R.exact_numerators(raw.indptr, raw.indices, raw.data, lut, pi, theta)
    kept = np.add.reduceat(inpat.astype(np.int64), raw.indptr[:-1])
    lens = np.diff(raw.indptr)
    assert lens[0] == 2 and kept[0] == 1 and kept[1] == 0 and lens[4] == 1 and kept[4] == 0
    assert np.any((kept == 1) & (lens > 2)) and np.any((kept > 1) & (kept < lens)) and np.any((kept == 0) & (lens > 1))
    assert np.any((kept < lens) & (lens > 64))                      # dead columns in rows of the long-row path
    raw, lut, pi, theta = R.dead_column_case('denormal')
    c = pi * theta
    assert np.any((c > 0) & (c < R.TINY)) and np.any((c == 0) & (pi > 0) & (theta > 0))
    raw, lut, pi, theta = R.dead_column_case('zero_score')
    assert np.any(raw.data == 0) and lut[0] > 0
    assert sp.csr_matrix(raw).nnz == len(raw.data)
