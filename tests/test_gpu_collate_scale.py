"""`--collate device` on the GPU at the sizes of tests/_collate_streams.py: every sort path of rocprim::radix_sort_keys on both sides
of its limit (one block up to 1,024 keys, merge sort up to 2^20, Onesweep above), the top bit of `bits` at n = 2^k + 1, one slot
contended by 300,001 lanes and one chain walked by 120,000, probe chains of 16 names, all 64 (source & 3, destination & 3, length & 3)
paths of k_collate_gather for W = 16 and W = 64 and the width switch on both sides, rec_off[0] != 0 and bytes behind rec_off[n],
several refused records in different blocks.

Every stream runs twice on the device; both runs must equal collate_np (the numpy definition, which shares nothing with the C
bodies) and tsem_bam_collate_host in `order`, the number of names and the bytes.  Everything is exact.  A failure names the side (the
host entry equals the definition and the device does not: the kernels; the host entry differs: a shared body, or the definition)
and the stage.  `pytest -s` prints the device's five `ms` figures per stream as `COLLATE_SCALE` lines (profiles/r35_collate_scale.txt
keeps a run).  tests/test_collate_streams_host.py holds the streams to what they claim without a GPU."""
import functools

import numpy as np
import pytest

import _collate_streams as S

pytestmark = pytest.mark.gpu
MS_KEYS = ['d2h', 'gather', 'h2d', 'hash_insert_key', 'sort_scan']
_faulted = []                                     # HIP errors met so far: after one, nothing more is started on the device


@pytest.fixture(autouse=True)
def _nothing_after_a_fault():
    if _faulted:
        pytest.fail('an earlier test of this file met a HIP error (%s): no further work is started on the device' % _faulted[0])
    yield


def _device(data, off, gpu_device, bits=0):
    """_lib.bam_collate on the device; a HIP error (TSEM_ERR_HIP, TSEM_ERR_TIMEOUT) is remembered for the fixture above"""
    from telescope_amd import _lib
    try:
        return _lib.bam_collate(data, off, device=gpu_device, hash_bits=bits)
    except _lib.EngineError as e:
        if getattr(e, 'code', None) in (-2, -4):
            _faulted.append(str(e))
        raise


@functools.lru_cache(maxsize=None)
def _host(name, bits):
    from telescope_amd import _lib
    data, off = S.get(name)
    out, order, names, _ = _lib.bam_collate(data, off, device=None, hash_bits=bits)
    return out, order, names


def _differs(name, got, ref):
    """None, or (stage, words) of the first thing in which (out, order, names) differs from the definition"""
    data, off = S.get(name)
    out, order, names = got
    if not np.array_equal(order, ref.order):
        return 'hash, insert, key or sort', 'order differs, ' + S.describe_order(ref.order, order, S.group_first(data, off)[0])
    if names != ref.n_names:
        return 'insert or key', 'order is equal, n_names is %d, the definition has %d' % (names, ref.n_names)
    if not np.array_equal(out, ref.out):
        return 'gather', 'order is equal, the bytes differ, ' + S.describe_bytes(off, ref.order, ref.out_off, ref.out, out)
    return None


def _hold(name, bits, gpu_device):
    """both device runs against the definition and the host entry -> the two outputs"""
    data, off = S.get(name)
    ref = S.reference(name)
    host = _host(name, bits)
    host_bad = _differs(name, host, ref)
    outs = []
    for run in (1, 2):                                       # the same input twice in one process: the races fall differently
        out, order, names, ms = _device(data, off, gpu_device, bits)
        where = '%s, %d records, hash_bits %d, run %d' % (name, len(off) - 1, bits, run)
        print('COLLATE_SCALE %s ms %s' % (where, ' '.join('%s %.3f' % (k, ms[k]) for k in ('h2d', 'hash_insert_key', 'sort_scan', 'gather', 'd2h'))), flush=True)
        bad = _differs(name, (out, order, names), ref)
        if host_bad is None:
            assert bad is None, 'the host entry equals the definition, the device does not: the kernels (%s): %s: %s' % (bad[0], where, bad[1])
        assert host_bad is None, ('the host entry differs from the definition: a shared body of tsem_bam_collate.h, or the definition (%s): %s: %s; '
                                  'the device %s' % (host_bad[0], where, host_bad[1], 'equals the definition' if bad is None else 'differs too: ' + bad[1]))
        assert np.array_equal(order, host[1]) and names == host[2] and np.array_equal(out, host[0]), 'device and host entry differ: ' + where
        assert sorted(ms) == MS_KEYS and all(v >= 0 for v in ms.values()), where
        outs.append(out)
    return outs


@pytest.mark.parametrize('name,bits', S.RUNS, ids=S.RUN_IDS)
def test_device_equals_the_definition_and_the_host(name, bits, gpu_device):
    _hold(name, bits, gpu_device)


def test_the_width_switch_changes_nothing_but_the_trimmed_record(gpu_device):
    """width_1023 (W = 16) and width_1024 (W = 64) hold the same records except for the last input record, one byte longer in the
    second: the two outputs are the same record by record, except for that record's block_size and its one byte more"""
    assert (S.gather_width(S.get('width_1023').off), S.gather_width(S.get('width_1024').off)) == (16, 64)
    a = _hold('width_1023', 0, gpu_device)[1]
    b = _hold('width_1024', 0, gpu_device)[1]
    ra, rb = S.reference('width_1023'), S.reference('width_1024')
    n = len(ra.order)
    k = int(np.flatnonzero(ra.order == n - 1)[0])
    assert np.array_equal(ra.order, rb.order) and np.array_equal(ra.out_off[:k + 1], rb.out_off[:k + 1])
    assert np.array_equal(ra.out_off[k + 1:] + 1, rb.out_off[k + 1:]) and 0 < k < n - 1
    assert np.array_equal(a[:ra.out_off[k]], b[:rb.out_off[k]]), 'the records in front of the trimmed one'
    assert np.array_equal(a[ra.out_off[k + 1]:], b[rb.out_off[k + 1]:]), 'the records behind the trimmed one'
    assert np.array_equal(a[ra.out_off[k] + 4:ra.out_off[k + 1]], b[rb.out_off[k] + 4:rb.out_off[k + 1] - 1]), 'the trimmed record'
    size_a, size_b = (int.from_bytes(x[o:o + 4].tobytes(), 'little') for x, o in ((a, ra.out_off[k]), (b, rb.out_off[k])))
    assert size_a + 1 == size_b == rb.out_off[k + 1] - rb.out_off[k] - 4


@pytest.mark.parametrize('name', S.REFUSED)
def test_device_reports_the_earliest_of_several_refused_records(name, gpu_device):
    """three malformed records in three different blocks of k_collate_hash: the report is the earliest one's, with its own code"""
    from telescope_amd import _lib
    data, off, bad, code = S.refused(name)
    for _run in (1, 2):
        with pytest.raises(ValueError) as e:
            _device(data, off, gpu_device)
        assert str(e.value) == 'record %d: %s' % (bad, _lib.COLLATE_STATUS[code])


@pytest.mark.parametrize('lead,trail', S.LEAD_TRAIL)
def test_device_accepts_bytes_in_front_of_the_first_record_and_behind_the_last(lead, trail, gpu_device):
    """rec_off[0] != 0 and bytes behind rec_off[n] (the accepted set of col_args): gather_narrow's groups and lengths, so the same
    order and output offsets, with every source alignment shifted by `lead`; the output begins with the first record, not the lead"""
    name = 'lead_trail_%d_%d' % (lead, trail)
    data, off = S.get(name)
    assert off[0] == lead and len(data) - off[-1] == trail
    out = _hold(name, 0, gpu_device)[1]
    ref, narrow = S.reference(name), S.reference('gather_narrow')
    assert np.array_equal(ref.order, narrow.order) and np.array_equal(ref.out_off, narrow.out_off) and len(out) == off[-1] - lead
    first = int(ref.order[0])
    assert np.array_equal(out[:ref.out_off[1]], data[off[first]:off[first + 1]])
