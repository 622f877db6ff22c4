"""One handle of the device loader's units (telescope_amd/csrc/tsem_stage.h under tsem_bgzf.hip, tsem_bam.hip, tsem_bam_collate.hip) driven
through calls of changing size — small, large, small, middle — where "large" is far more than 1.25 times "small": the second call must
reallocate every buffer, the third runs inside buffers larger than it needs.  A stale capacity, a buffer that did not grow with its
partner, a stage clock or a status word that carries over from the call before shows here; every call is held to the reference that
the tests of the unit itself use (zlib, tsem_bgzf_deflate_host, _loader_reference.compare_stages, _bam_edit_reference,
tsem_bam_collate_host).  No tolerance anywhere."""
import functools
import struct

import numpy as np
import pytest

import _bam_edit_reference as ed
import _bam_fuzz as fuzz
import _bgzf_reference as bref
import _collate_reference as cr
import _loader_reference as lref
from telescope_amd import _lib
from telescope_amd import loader
from telescope_amd import loader_device as ld

pytestmark = pytest.mark.gpu
BLOCK = _lib.BGZF_BLOCK_IN
NFK = '__no_feature'


def _counts_and_reset(times, count_key, calls):
    """the stage clock behind a *_times entry: `calls` calls so far, no negative time; after a reset zeros and 0"""
    t = times()
    assert t.pop(count_key) == calls and all(v >= 0 for v in t.values()) and any(v > 0 for v in t.values()), t
    assert times(reset=True)[count_key] == calls
    t = times()
    assert t.pop(count_key) == 0 and all(v == 0 for v in t.values()), t


# ------------------------------------------------------------------------------------------------------------------- BgzfInflater
def test_inflater_through_batches_of_changing_size(gpu_device):
    v, big = bref.zlib_made(), bref.oversize_case()
    by = {c.name: c for c in v + bref.hand_built_valid()}
    batches = [[by['one_byte']],
               [by['size_65280'], by['incompressible'], big, by['level0_stored'], by['sync_flush'], by['empty']],   # (big: left to the host)
               [by['sync_flush']],
               [by['level6'], by['hand_fixed_285_dist_32768'], by['one_byte']]]
    assert [len(b) for b in batches] == [1, 6, 1, 3]
    dev = _lib.BgzfInflater(gpu_device)
    try:
        for cs in batches:
            data = b''.join(bref.case_block(c) for c in cs)
            blocks, used, not_bgzf = _lib.bgzf_scan(data)
            assert used == len(data) and not not_bgzf and len(blocks) == len(cs)
            out, st, first = dev.inflate(data, blocks)
            assert st.tolist() == [bref.ST_HOST if c is big else 0 for c in cs] and first == (0, -1)
            assert out.tobytes() == b''.join(c.expected for c in cs if c is not big)
        _counts_and_reset(dev.times, 'batches', 4)
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------------------------- BgzfDeflater
def test_deflater_through_streams_of_changing_size(gpu_device):
    rng = np.random.RandomState(34)
    words = [bytes(rng.randint(65, 91, rng.randint(2, 12)).astype(np.uint8)) for _ in range(200)]
    text = b' '.join(words[i] for i in rng.randint(0, 200, 3 * BLOCK // 4))
    assert len(text) > 3 * BLOCK
    dev = _lib.BgzfDeflater(gpu_device)
    try:
        for k, n in enumerate([1, 3 * BLOCK + 1, BLOCK, BLOCK + 1]):
            stream = text[k:k + n]                           # (another cut of the text every time: no block repeats the call before)
            assert dev.deflate(stream).tobytes() == _lib.bgzf_deflate_host(stream).tobytes(), n
        _counts_and_reset(dev.times, 'batches', 4)
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------------------- BamLoader: the chunks
MODE = 'None'                                                # (fuzz case 0: test_gpu_device_loader.MODES[0])


@pytest.fixture(scope='module')
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp('stage_reuse'))


@functools.lru_cache(maxsize=None)
def _case(directory):
    """fuzz case 0 of test_gpu_device_loader: (case, stage reference, annotation)"""
    c = fuzz.make_case(0, directory)
    ref, ann = lref.reference(c.bam, c.gtf, MODE, 'CB', 'UB')
    return c, ref, ann


@functools.lru_cache(maxsize=None)
def _chunks(bam, max_bundles):
    import gzip
    import io
    with io.BufferedReader(gzip.open(bam, 'rb')) as fh:
        loader.read_bam_header(fh, bam)
        return tuple((bytes(d), np.array(o)) for d, o in ld.bam_chunks(fh, bam, ld.DEFAULT_CHUNK_BYTES, max_bundles))


def _open_loader(gpu_device, ann, refs):
    arrs = ld.annotation_arrays(ann, refs)
    dev = _lib.BamLoader(gpu_device, *arrs[:-1])
    dev.names(arrs[-1] + [NFK])
    return dev


def _run_chunk(dev, ann, data, off):
    return dev.chunk(data, off, 'CB', 'UB', ann.run_stranded, MODE, 0.2, fuzz.RECORD_CAP)


def _whole_matrix(dev, ann, chunks):
    """the chunks one after the other on the handle -> their matrices as one, record indices of the file (test_stage_parity_names_the_kernel)"""
    base, parts = 0, []
    for data, off in chunks:
        out, st = _run_chunk(dev, ann, data, off)
        assert st == (0, -1)
        out = out.copy()
        for col in (ld.C_PAIR1, ld.C_PAIR2, ld.C_BUNDLE):
            out[col][out[col] >= 0] += base
        parts.append(out)
        base += out.shape[1]
    return np.concatenate(parts, axis=1)


def _check_matrix(c, ref, ann, mat):
    hosted = np.flatnonzero(mat[ld.C_BCLASS] == ld.CLS_HOST).tolist()
    assert len(hosted) == c.expected_fallbacks
    lref.compare_stages(ref, ann, mat, host_expected=hosted)


def test_loader_through_chunks_of_changing_size_and_a_reported_record(gpu_device, workdir):
    from test_gpu_device_loader import _malformed_bam
    c, ref, ann = _case(workdir)
    one, whole, some = _chunks(c.bam, 1), _chunks(c.bam, None), _chunks(c.bam, 7)
    assert len(whole) <= 2 and len(one) > 2 * len(some) > 8
    n_max = max(len(off) - 1 for _d, off in one)
    assert len(whole[0][1]) - 1 > 2 * n_max + 8 and len(whole[0][0]) > 2 * max(len(d) for d, _o in one) + 8   # (large: it must reallocate)
    bad_bam, _gtf, k, _name = _malformed_bam(workdir, 'z_without_nul')
    _refs, bad_data, bad_off = lref.inflated_records(bad_bam)
    code, = [s for s, text in _lib.BAM_STATUS.items() if 'no NUL inside the record' in text]
    dev = _open_loader(gpu_device, ann, ref.refs)
    try:
        for chunks in (one, whole, one):
            _check_matrix(c, ref, ann, _whole_matrix(dev, ann, chunks))
        _out, st = _run_chunk(dev, ann, bad_data, bad_off)   # the walk stops at the record's end and lowers the status word
        assert st == (code, k)
        _check_matrix(c, ref, ann, _whole_matrix(dev, ann, some))          # ... which the next call finds armed again
        _counts_and_reset(dev.times, 'chunks', 2 * len(one) + len(whole) + 1 + len(some))
    finally:
        dev.close()


# -------------------------------------------------------------------------------------------------------- BamLoader: the rewriting
@functools.lru_cache(maxsize=None)
def _load_streams(directory):
    """(other, tmp) of fuzz case 0 by the host program of _bam_edit_reference, the file as one chunk"""
    c, _ref, ann = _case(directory)
    exe = ed.build_host_program(directory)
    other, tmp, hosted = ed.host_load(exe, c.bam, ann, MODE, NFK, fuzz.RECORD_CAP, directory)
    assert hosted == c.expected_fallbacks
    return other, tmp


def _device_streams(dev, ann, refs, chunks):
    """the load stage of the chunks one after the other -> (other, tmp, sizing calls): the device's streams, the bundles left to the host
    spliced in at their offsets as load_alignment_device does"""
    assign = lambda pair: loader.assign_pair(pair, ann, refs, MODE, NFK, 0.2)
    pieces = ([], [])
    for data, off in chunks:
        out, st = _run_chunk(dev, ann, data, off)
        assert st == (0, -1)
        n = len(off) - 1
        pos_o, pos_t, st = dev.rewrite_size(n)
        assert st == (0, -1)
        kind, _pair = dev.rewrite_slots(n)
        streams = dev.rewrite_fetch(pos_o[n], pos_t[n])
        assert int(np.count_nonzero(kind == 1)) == _n_framed(streams[0]) and int(np.count_nonzero(kind >= 2)) == _n_framed(streams[1])
        starts = np.flatnonzero(out[ld.C_BITS] & ld.BIT_NEWNAME).tolist()
        at = [0, 0]
        for b, s in enumerate(starts):
            if out[ld.C_BCLASS][s] != ld.CLS_HOST:
                continue
            h = ld.host_bundle(data, off, s, starts[b + 1] if b + 1 < len(starts) else n, None, None, assign, NFK, streams=True)
            for j, (pos, piece) in enumerate(((int(pos_o[s]), h['other']), (int(pos_t[s]), h['tmp']))):
                pieces[j].extend([streams[j][at[j]:pos].tobytes(), piece]); at[j] = pos
        for j in (0, 1):
            pieces[j].append(streams[j][at[j]:].tobytes())
    return b''.join(pieces[0]), b''.join(pieces[1])


def _frames(stream):
    """rec_off int64 [n + 1] of a stream of framed records"""
    off, p = [0], 0
    while p < len(stream):
        p += 4 + struct.unpack_from('<i', stream, p)[0]
        off.append(p)
    assert p == len(stream)
    return np.array(off, np.int64)


def _n_framed(stream):
    return len(_frames(stream.tobytes())) - 1


def test_rewrite_through_chunks_of_changing_size_then_an_update_larger_than_all(gpu_device, workdir):
    c, ref, ann = _case(workdir)
    want = _load_streams(workdir)
    one, whole = _chunks(c.bam, 1), _chunks(c.bam, None)
    dev = _open_loader(gpu_device, ann, ref.refs)
    try:
        for chunks in (one, whole, one):
            assert _device_streams(dev, ann, ref.refs, chunks) == want
        sizings = 2 * len(one) + len(whole)
        # ---- the update stage on a tmp stream of more records and more bytes than any chunk so far: it reuses the chunk's buffers
        (data, off), tmp = whole[0], want[1]
        reps = max(2 * (len(off) - 1) // (len(_frames(tmp)) - 1), 2 * len(data) // len(tmp)) + 1
        stream = tmp * reps
        s_off = _frames(stream)
        n = len(s_off) - 1
        assert n > 2 * (len(off) - 1) and len(stream) > 2 * len(data)
        pool = [ed.word(ed.KEEP), ed.word(ed.SEC), ed.word(ed.SEC, 77, 50, True, True), ed.word(ed.PRI, 0, 0), ed.word(ed.PRI, 255, 100, True, True),
                ed.word(ed.PRI, 13, 19, False, False), ed.word(ed.PRI, 160, 99, True, False)]
        words = np.array([pool[i % len(pool)] for i in range(n)], np.uint32)
        expected = b''.join(ed.frame(ed.updated(stream[int(s_off[i]) + 4:int(s_off[i + 1])], int(words[i]))) for i in range(n))
        pos, st = dev.update_size(stream, s_off, words)
        assert st == (0, -1) and int(pos[n]) == len(expected)
        other, got = dev.rewrite_fetch(0, pos[n])
        assert other.size == 0 and got.tobytes() == expected
        # ---- the chunk's bytes were overwritten: a load-stage sizing behind an update is refused, not run on the update's records
        pos, st = dev.update_size(stream[:int(s_off[3])], s_off[:4], words[:3])
        assert st == (0, -1)
        with pytest.raises(_lib.EngineError) as e:
            dev.rewrite_size(3)
        assert e.value.code == _lib.ERR_ARG and 'no chunk on the device' in str(e.value)
        _counts_and_reset(dev.rewrite_times, 'calls', sizings + 2)        # (the sizing calls, of either stage; the refused one is none)
        assert dev.times()['chunks'] == sizings
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------------------------------ collate
def test_collate_twice_small_then_large(gpu_device, workdir):
    small = min((r for r in cr.cases().values() if 1 < len(r) < 64), key=lambda r: sum(map(len, r)))
    _refs, data, off = lref.inflated_records(fuzz.make_case(0, workdir).bam)
    large = cr.reordered(cr.split(data, off), 'shuffled')
    assert len(large) > 2 * len(small) + 8 and sum(map(len, large)) > 2 * sum(map(len, small)) + 8
    for records in (small, large):                          # (the unit keeps nothing: the second call owes nothing to the first)
        data, off = cr.stream_of(records)
        want, want_order, want_names, _ = _lib.bam_collate(data, off, device=None)
        got, order, names, ms = _lib.bam_collate(data, off, device=gpu_device)
        assert np.array_equal(order, want_order) and names == want_names and got.tobytes() == want.tobytes()
        assert sorted(ms) == ['d2h', 'gather', 'h2d', 'hash_insert_key', 'sort_scan'] and all(v >= 0 for v in ms.values())
