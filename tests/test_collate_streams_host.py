"""`--collate` without a GPU at the sizes of tests/_collate_streams.py: the streams are what they say (every sort path of rocprim on
both sides of its limit, the top bit of `bits`, all 64 alignments of the gather for both widths, long probe chains, one slot for
300,001 records), the vectorised definition collate_np equals the written one of _collate_reference, and tsem_bam_collate_host — the
bodies the kernels share — equals collate_np on every stream, the 2^20 ones included."""
import numpy as np
import pytest

import _collate_reference as cr
import _collate_streams as S
from telescope_amd import _lib

ALL_COMBOS = {(s, d, ln) for s in range(4) for d in range(4) for ln in range(4)}
SMALL = [name for name in S.STREAMS if name.startswith(('edge_n', 'single_block', 'merge_1025', 'gather', 'last_byte', 'width', 'lead_trail'))]


def _n(name):
    return len(S.get(name).off) - 1


def _combos(name):
    return S.alignment_combos(S.get(name).off, S.reference(name).order, S.reference(name).out_off)


# ------------------------------------------------------------------------------------------------ the streams are what they say
def test_the_sizes_sit_on_both_sides_of_every_limit():
    assert [_n('edge_n_%d' % n) for n in S.EDGE_N] == [1, 2, 3, 63, 64, 65, 255, 256, 257]
    assert (S.SINGLE_BLOCK_LIMIT, S.MERGE_SORT_LIMIT) == (1024, 1 << 20)
    assert _n('single_block_1024') == S.SINGLE_BLOCK_LIMIT and _n('merge_1025') == S.SINGLE_BLOCK_LIMIT + 1
    assert _n('merge_2p20') == S.MERGE_SORT_LIMIT and _n('onesweep_2p20p1') == _n('onesweep_zipf') == S.MERGE_SORT_LIMIT + 1
    for name in S.IDENTITY:
        assert S.SINGLE_BLOCK_LIMIT < _n(name) == 300001 <= S.MERGE_SORT_LIMIT
    assert _n('chains_bits8') == _n('chains_bits12') == 20000 and _n('gather_narrow') == 5000 and _n('gather_wide') == 4096
    assert dict(S.RUNS)['chains_bits8'] == 8 and dict(S.RUNS)['chains_bits12'] == 12 and ('gather_narrow', 4) in S.RUNS and ('gather_narrow', 0) in S.RUNS


@pytest.mark.parametrize('name', S.POW2_PLUS_1)
def test_the_last_record_of_a_2_k_plus_1_stream_needs_the_top_bit(name):
    data, off = S.get(name)
    n = len(off) - 1
    assert n > 2 and (n - 1) & (n - 2) == 0                                  # n = 2^k + 1: n - 1 is the one index with bit k set
    first, _ = S.group_first(data, off)
    assert first[n - 1] == n - 1 and S.reference(name).order[n - 1] == n - 1


def test_the_pairs_are_pairs():
    for name in ('single_block_1024', 'merge_1025', 'merge_2p20', 'onesweep_2p20p1'):
        n = _n(name)
        assert S.reference(name).n_names == (n + 1) // 2
        first, _ = S.group_first(*S.get(name))
        sizes = np.bincount(first)
        assert np.array_equal(np.bincount(sizes[sizes > 0]), [0, n & 1, n // 2])           # groups of 1 and of 2 records
    lens = np.diff(S.get('merge_2p20').off)
    assert lens.min() == 38 and lens.max() == 36 + 40 + 1 + 23


def test_the_zipf_stream_has_one_group_all_over_the_stream():
    data, off = S.get('onesweep_zipf')
    n = len(off) - 1
    first, names = S.group_first(data, off)
    sizes = np.bincount(first)
    big = int(np.argmax(sizes))
    members = np.flatnonzero(first == big)
    assert sizes[big] >= 100000 and members[0] < n // 100 and members[-1] >= n - n // 100
    rest = sizes[(sizes > 0) & (np.arange(n) != big)]
    assert np.count_nonzero(rest == 1) > len(rest) // 3 and rest.max() <= 64 and names == len(rest) + 1


def test_the_identity_streams_are_collated_already():
    want_names = {'one_name_300001': 1, 'all_distinct_300001': 300001}
    for name in S.IDENTITY:
        data, off = S.get(name)
        ref = S.reference(name)
        assert np.array_equal(ref.order, np.arange(len(off) - 1)) and np.array_equal(ref.out, data)
        assert ref.n_names == want_names.get(name, ref.n_names)
    first, groups = S.group_first(*S.get('already_collated_300001'))
    assert 300001 // 4 <= groups == S.reference('already_collated_300001').n_names < 300001 and np.all(np.diff(first) >= 0)


def test_the_gather_streams_visit_every_alignment_on_both_sides_of_the_width():
    for name, width in (('gather_narrow', 16), ('gather_wide', 64)):
        assert _combos(name) == ALL_COMBOS, (name, sorted(ALL_COMBOS - _combos(name)))
        assert S.gather_width(S.get(name).off) == width
    off = S.get('gather_narrow').off
    assert int(off[-1] - off[0]) // (len(off) - 1) < 1024
    off = S.get('gather_wide').off
    lens = np.diff(off)
    assert int(off[-1] - off[0]) // (len(off) - 1) >= 1024
    assert lens.min() == 37 and lens.max() == 70001 > 65536
    small = np.count_nonzero(lens <= 44)
    assert 0.25 < small / len(lens) < 0.35 and np.all((lens <= 44) | ((lens >= 900) & (lens <= 2400)) | (lens == 70001))
    for lead, trail in S.LEAD_TRAIL:
        name = 'lead_trail_%d_%d' % (lead, trail)
        data, off = S.get(name)
        assert off[0] == lead and len(data) - off[-1] == trail and _combos(name) == ALL_COMBOS
        assert np.array_equal(np.diff(off), np.diff(S.get('gather_narrow').off))


def test_the_width_streams_differ_in_one_byte_of_one_record():
    (d0, o0), (d1, o1) = S.get('width_1023'), S.get('width_1024')
    n = len(o0) - 1
    assert len(o1) - 1 == n and int(o0[n]) // n == 1023 and int(o1[n]) // n == 1024 and o1[n] == 1024 * n == o0[n] + 1
    assert (S.gather_width(o0), S.gather_width(o1)) == (16, 64)
    assert np.array_equal(o0[:n], o1[:n])
    # every record but the last is the same; the last is one byte shorter (its block_size says so) and otherwise the same
    assert np.array_equal(d0[:o0[n - 1]], d1[:o1[n - 1]]) and np.array_equal(d0[o0[n - 1] + 4:], d1[o1[n - 1] + 4:-1])
    k0, k1 = (int(np.flatnonzero(S.reference(w).order == n - 1)[0]) for w in ('width_1023', 'width_1024'))
    assert k0 == k1 < n - 1 and np.array_equal(S.reference('width_1023').order, S.reference('width_1024').order)


def test_the_chains_are_long():
    data, off = S.get('chains_bits8')
    assert S.reference('chains_bits8').n_names == 4096 >= 8 * 2 ** 8
    assert np.array_equal(S.get('chains_bits12').data, data)
    l = data[off[:-1] + 12].astype(int) - 1
    assert l.min() == 1 and l.max() == 254


def test_the_names_differ_in_their_last_bytes_and_hold_no_nul():
    data, off = S.get('gather_narrow')
    at = off[:-1]
    l = data[at + 12].astype(np.int64)
    long_ = l > 6
    assert np.all(data[at[long_] + 36] == S.FILLER) and np.all(data[at + 36 + l - 1] == 0)
    for j in range(int(l.max()) - 1):
        assert np.all(data[at[l - 1 > j] + 36 + j] != 0)
    size = data[at].astype(np.int64) | data[at + 1].astype(np.int64) << 8 | data[at + 2].astype(np.int64) << 16 | data[at + 3].astype(np.int64) << 24
    assert np.array_equal(size + 4, np.diff(off))
    # every other byte is random: of the fixed bytes 4 .. 11 and 13 .. 35 each takes (nearly) every value
    for b in (4, 11, 13, 35):
        assert len(np.unique(data[at + b])) > 250


def test_names_that_differ_in_the_last_of_their_l_read_name_bytes_are_different_names():
    (data, off), (d0, o0) = S.get('last_byte_5000'), S.get('gather_narrow')
    at = off[:-1]
    last = at + 36 + data[at + 12].astype(np.int64) - 1
    assert np.array_equal(off, o0) and np.array_equal(np.flatnonzero(data != d0), np.sort(last[data[last] != 0]))
    first, first0 = S.group_first(data, off)[0], S.group_first(d0, o0)[0]
    n = len(at)
    same_before = first0[first] == first0                                  # (a group only ever splits)
    assert np.all(same_before) and S.reference('gather_narrow').n_names + 500 < S.reference('last_byte_5000').n_names < n
    # some groups were split by that byte alone, others stayed together
    sizes, sizes0 = np.bincount(first, minlength=n), np.bincount(first0, minlength=n)
    assert np.count_nonzero((sizes0 > 1) & (sizes == sizes0)) > 100 and np.count_nonzero((sizes0 > 1) & (sizes < sizes0)) > 100


@pytest.mark.parametrize('name', [k for k in S.STREAMS if k not in S.IDENTITY and k not in ('edge_n_1', 'edge_n_2', 'edge_n_3')])
def test_a_stream_moves_at_least_half_of_its_records(name):
    order = S.reference(name).order
    assert 2 * np.count_nonzero(order != np.arange(len(order))) >= len(order)


# ------------------------------------------------------------------------------------- the fast definition and the written one
def _same_as_written(data, off, label):
    recs = cr.split(bytes(data), off)
    want, want_order = cr.collate(recs)
    out, order, names, out_off = S.collate_np(data, off)
    assert order.tolist() == want_order, label
    assert out.tobytes() == b''.join(want), label
    assert names == len({cr.name_of(r) for r in recs}), label
    assert np.array_equal(np.diff(out_off), [len(r) for r in want]), label


@pytest.mark.parametrize('label', list(cr.cases()))
def test_collate_np_equals_the_written_definition_on_the_built_cases(label):
    data, off = cr.stream_of(cr.cases()[label])
    _same_as_written(np.frombuffer(data, np.uint8), off, label)


@pytest.mark.parametrize('name', SMALL)
def test_collate_np_equals_the_written_definition_on_the_small_streams(name):
    data, off = S.get(name)
    assert len(off) - 1 <= 5000
    _same_as_written(data, off, name)


def test_every_stream_of_at_most_5000_records_is_held_to_the_written_definition():
    assert sorted(SMALL) == sorted(k for k in S.STREAMS if _n(k) <= 5000)


# ------------------------------------------------------------------------------------------- the shared bodies on the host
@pytest.mark.parametrize('name,bits', S.RUNS, ids=S.RUN_IDS)
def test_host_equals_collate_np(name, bits):
    data, off = S.get(name)
    ref = S.reference(name)
    out, order, names, ms = _lib.bam_collate(data, off, device=None, hash_bits=bits)
    assert ms is None
    assert np.array_equal(order, ref.order), 'order: ' + S.describe_order(ref.order, order, S.group_first(data, off)[0])
    assert names == ref.n_names
    assert np.array_equal(out, ref.out), 'bytes: ' + S.describe_bytes(off, ref.order, ref.out_off, ref.out, out)


@pytest.mark.parametrize('name', S.REFUSED)
def test_host_reports_the_earliest_of_several_refused_records(name):
    data, off, bad, code = S.refused(name)
    assert bad == S.REFUSED_AT[0] == 257 and code == 1 + S.REFUSED.index(name) and len(off) - 1 == 5000
    codes = [_check_code(data[off[i]:off[i + 1]]) for i in S.REFUSED_AT]
    assert sorted(codes) == [1, 2, 3] and codes[0] == code                 # the three kinds, this arrangement's own in front
    assert all(_check_code(data[off[i]:off[i + 1]]) == 0 for i in (0, 256, 258, 2599, 2601, 4998))
    with pytest.raises(ValueError) as e:
        _lib.bam_collate(data, off, device=None)
    assert str(e.value) == 'record %d: %s' % (bad, _lib.COLLATE_STATUS[code])


def _check_code(rec):
    """bam_collate_check, written again"""
    if len(rec) < 37:
        return 1
    if rec[12] == 0:
        return 2
    return 3 if 36 + int(rec[12]) > len(rec) else 0


# ------------------------------------------------------------------------------------------- the bodies, sanitized, on the host
@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    return cr.build_host_program(str(tmp_path_factory.mktemp('bam_collate_streams')))


@pytest.mark.parametrize('name,bits', [('gather_narrow', 4), ('chains_bits8', 8)])
def test_sanitized_program_on_two_streams(name, bits, exe, tmp_path):
    data, off = S.get(name)
    ref = S.reference(name)
    got, order, names = cr.host_run(exe, cr.split(bytes(data), off), bits, str(tmp_path), name)
    assert order == ref.order.tolist() and names == ref.n_names and got == ref.out.tobytes()


# ------------------------------------------------------------------------------------------- the words of a failure
def test_the_failure_words_name_what_is_wrong():
    data, off = S.get('merge_1025')
    ref = S.reference('merge_1025')
    first = S.group_first(data, off)[0]
    n = len(ref.order)
    # the last record sorted as if its top bit were not there: still grouped
    assert ref.order[0] == 0 and first[ref.order[1]] == 0
    low = np.r_[ref.order[:2], n - 1, ref.order[2:-1]]
    text = S.describe_order(ref.order, low, first)
    assert 'still a permutation: True' in text and 'still grouped: True' in text and 'record %d' % (n - 1) in text
    torn = ref.order.copy()
    torn[[1, n - 1]] = torn[[n - 1, 1]]
    assert 'still grouped: False' in S.describe_order(ref.order, torn, first)
    twice = ref.order.copy()
    twice[5] = twice[4]
    assert 'still a permutation: False' in S.describe_order(ref.order, twice, first)
    k = 700
    wrong = ref.out.copy()
    wrong[ref.out_off[k] + 9] ^= 1
    i = int(ref.order[k])
    want = '(%d, %d, %d), length %d, W = 16' % (off[i] & 3, ref.out_off[k] & 3, (off[i + 1] - off[i]) & 3, off[i + 1] - off[i])
    text = S.describe_bytes(off, ref.order, ref.out_off, ref.out, wrong)
    assert 'byte 9 of output record %d (input record %d)' % (k, i) in text and want in text
