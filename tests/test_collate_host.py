"""`--collate` without a GPU: tsem_bam_collate_host and the same bodies in a stand-alone program under the address and
undefined-behaviour sanitizers (tests/c_host/bam_collate_check.cc: every record in a heap block of exactly its size) against the
definition in _collate_reference.collate, on bytes and on `order`; the refusals of malformed records; the CLI's refusals and defaults."""
import os

import numpy as np
import pytest

import _collate_reference as cr
import _loader_reference as lr
from telescope_amd import _lib, cli, loader

CASES = cr.cases()


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    return cr.build_host_program(str(tmp_path_factory.mktemp('bam_collate')))


@pytest.fixture(scope='module')
def file_cases(tmp_path_factory):
    """label -> framed records of the fixture and fuzz BAMs, sorted by (ref, pos) and shuffled"""
    d = str(tmp_path_factory.mktemp('collate_files'))
    out = {}
    for src in cr.sources(d):
        _refs, data, off = lr.inflated_records(src[1])
        recs = cr.split(data, off)
        for how in ('sorted', 'shuffled'):
            out['%s-%s' % (src[0], how)] = cr.reordered(recs, how, seed=len(src[0]))
    return out


def _host(records, bits):
    data, off = cr.stream_of(records)
    out, order, names, ms = _lib.bam_collate(data, off, device=None, hash_bits=bits)
    assert ms is None
    return out.tobytes(), order.tolist(), names


def _check(records, bits, label):
    want, want_order = cr.collate(records)
    got, order, names = _host(records, bits)
    assert order == want_order, (label, bits)
    assert got == b''.join(want), (label, bits)
    assert names == len({cr.name_of(r) for r in records}), (label, bits)
    return got, order


@pytest.mark.parametrize('bits', cr.HASH_BITS)
@pytest.mark.parametrize('label', list(CASES))
def test_host_equals_the_definition_on_the_built_cases(label, bits):
    recs = CASES[label]
    got, order = _check(recs, bits, label)
    if label == 'already_collated':
        assert order == list(range(len(recs)))
    # collating the result a second time changes nothing
    data, off = cr.stream_of(cr.collate(recs)[0])
    again, order2, _ = _host(cr.split(data, off), bits)
    assert again == got and order2 == list(range(len(recs)))


def test_the_built_cases_are_what_they_say():
    c = CASES
    assert len(c['n0']) == 0 and len(c['n1']) == 1
    assert len({cr.name_of(r) for r in c['one_name']}) == 1 and len({cr.name_of(r) for r in c['all_distinct']}) == len(c['all_distinct'])
    assert {len(cr.name_of(r)) for r in c['name_lengths_1_254']} == {2, 255}
    assert {cr.name_of(r) for r in c['prefixes']} >= {b'r1\x00', b'r10\x00', b'r1' + b'x' * 250 + b'\x00'}
    names = {cr.name_of(r) for r in c['last_byte_differs']}
    assert len(names) == 4 and len({n[:-2] for n in names}) == 1
    sizes = [sum(cr.name_of(r) == n for r in c['groups_of_1_and_200']) for n in (b'solo\x00', b'big\x00')]
    assert sizes == [1, 200]
    fl = c['first_and_last']
    assert [i for i, r in enumerate(fl) if cr.name_of(r) == b'ends\x00'] == [0, len(fl) - 1]
    assert {len(r) % 4 for r in c['sizes_mod_4']} == {0, 1, 2, 3}
    assert min(len(r) for r in c['smallest']) == 37
    assert max(len(r) for r in c['above_128k']) > 128 << 10
    assert cr.collate(c['groups_of_1_and_200'])[1] != list(range(len(c['groups_of_1_and_200'])))


@pytest.mark.parametrize('bits', cr.HASH_BITS)
def test_host_equals_the_definition_on_reordered_files(file_cases, bits):
    assert len(file_cases) == 12
    for label, recs in file_cases.items():
        got, order = _check(recs, bits, label)
        assert order != list(range(len(recs))), label         # (the reordering did split groups)
        data, off = cr.stream_of(cr.split(*cr.stream_of(cr.collate(recs)[0])))
        again, order2, _ = _host(cr.split(data, off), bits)
        assert again == got and order2 == list(range(len(recs))), label


@pytest.mark.parametrize('label', list(cr.malformed()))
def test_a_malformed_record_is_refused_by_its_index(label):
    recs, bad, code = cr.malformed()[label]
    data, off = cr.stream_of(recs)
    with pytest.raises(ValueError) as e:
        _lib.bam_collate(data, off, device=None)
    assert str(e.value) == 'record %d: %s' % (bad, _lib.COLLATE_STATUS[code])


def test_the_arguments_are_checked_before_anything_is_read():
    data, off = cr.stream_of(CASES['prefixes'])
    worse = off.copy(); worse[3] = worse[2] - 1
    with pytest.raises(_lib.EngineError, match='offsets of record 2'):
        _lib.bam_collate(data, worse, device=None)
    past = off.copy(); past[-1] += 1
    with pytest.raises(_lib.EngineError, match='offsets of record %d' % (len(off) - 2)):
        _lib.bam_collate(data, past, device=None)
    with pytest.raises(_lib.EngineError, match='hash_bits'):
        _lib.bam_collate(data, off, device=None, hash_bits=65)
    # the device entry checks the same before it touches a device: 2^32 - 1 records are refused without one
    L = _lib.lib()
    names, st = _lib.C.c_int64(), np.zeros(2, np.int64)
    rc = L.tsem_bam_collate(0, None, 0, _lib.ptr(off), (1 << 32) - 1, 0, None, _lib.ptr(np.zeros(1, np.int64)), _lib.C.byref(names), _lib.ptr(st), None)
    assert rc == _lib.ERR_ARG and '2^32 - 1 records' in L.tsem_last_error(None).decode()


# ------------------------------------------------------------------------------------------- the bodies, sanitized, on the host
@pytest.mark.parametrize('bits', cr.HASH_BITS)
def test_sanitized_program_on_the_built_cases(exe, tmp_path, bits):
    for label, recs in CASES.items():
        want, want_order = cr.collate(recs)
        got, order, names = cr.host_run(exe, recs, bits, str(tmp_path), label)
        assert order == want_order and got == b''.join(want) and names == len({cr.name_of(r) for r in recs}), (label, bits)


def test_sanitized_program_on_reordered_files(exe, tmp_path, file_cases):
    for k, (label, recs) in enumerate(file_cases.items()):
        want, want_order = cr.collate(recs)
        got, order, _ = cr.host_run(exe, recs, cr.HASH_BITS[k % 3], str(tmp_path), label)
        assert order == want_order and got == b''.join(want), label


def test_sanitized_program_refuses_the_malformed_records(exe, tmp_path):
    for label, (recs, bad, code) in cr.malformed().items():
        assert cr.host_run(exe, recs, 0, str(tmp_path), label) == (code, bad), label


# ------------------------------------------------------------------------------------------------------- collate.collated_stream
def test_collated_stream_of_a_sorted_bam_reads_like_the_collated_file(tmp_path, caplog):
    import gzip
    import io
    import logging
    from telescope_amd import collate
    src = [s for s in cr.sources(str(tmp_path)) if s[0] == 'fuzz1'][0]
    p_in, p_ref, recs = cr.reordered_files(str(tmp_path), src, 'sorted')
    fh = io.BufferedReader(gzip.open(p_in, 'rb'))
    loader.read_bam_header(fh, p_in)
    with caplog.at_level(logging.INFO):
        s = collate.collated_stream(fh, p_in, 'host')
    got = b''
    for n in (1, 3, 4096, 7, 1 << 20):                         # read(n) in uneven pieces, then to the end
        got += s.read(n)
    while True:
        b = s.read(5000)
        if not b:
            break
        got += b
    s.close()
    assert fh.closed and s.read(10) == b''
    assert got == lr.inflated_records(p_ref)[1] == b''.join(cr.collate(recs)[0])
    want_moved = sum(i != k for k, i in enumerate(cr.collate(recs)[1]))
    assert collate.LAST['records'] == len(recs) and collate.LAST['moved'] == want_moved > 0 and collate.LAST['ms'] is None
    assert collate.LAST['names'] == len({cr.name_of(r) for r in recs})
    line = [r.getMessage() for r in caplog.records if r.getMessage().startswith('collate (host)')]
    assert len(line) == 1 and '%d records, %d names, %d records moved' % (len(recs), collate.LAST['names'], want_moved) in line[0]
    with pytest.raises(ValueError, match="collate must be"):
        collate.collated_stream(io.BytesIO(b''), 'x', 'none')


def test_collated_stream_names_the_file_of_a_truncated_or_malformed_stream():
    import io
    from telescope_amd import collate
    good = b''.join(CASES['prefixes'])
    with pytest.raises(ValueError, match='cut.bam: truncated BAM'):
        collate.collated_stream(io.BytesIO(good[:-5]), 'cut.bam', 'host')
    recs, bad, code = cr.malformed()['l_read_name_0']
    with pytest.raises(ValueError) as e:
        collate.collated_stream(io.BytesIO(b''.join(recs)), 'bad.bam', 'host')
    assert str(e.value) == 'bad.bam: record %d: %s' % (bad, _lib.COLLATE_STATUS[code])


# ------------------------------------------------------------------------------------------------------------------ the CLI
def _assign(*more):
    return ['assign', os.path.join(cr.GOLD, 'loader_mixed.bam'), os.path.join(cr.GOLD, 'loader_mixed.gtf')] + list(more)


def test_cli_collate_defaults_to_none():
    for argv in (_assign(), ['sc'] + _assign()):
        assert cli.build_parser().parse_args(argv).collate == 'none'
    assert cli.build_parser().parse_args(_assign('--collate', 'device')).collate == 'device'
    assert cli.build_parser().parse_args(['sc'] + _assign('--collate', 'host')).collate == 'host'
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(_assign('--collate', 'gpu'))


@pytest.mark.parametrize('sc', [False, True])
@pytest.mark.parametrize('how', ['host', 'device'])
def test_cli_collate_refusals_come_before_anything_is_read(tmp_path, sc, how):
    out = str(tmp_path / 'never')
    head = ['sc'] if sc else []
    with pytest.raises(SystemExit) as e:
        cli.main(head + _assign('--collate', how, '--outdir', out))
    assert '--collate %s without --loader device is not supported' % how in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(head + _assign('--collate', how, '--loader', 'device', '--updated_sam', '--outdir', out))
    assert '--collate %s with --updated_sam is not supported' % how in str(e.value) and 'run the two separately' in str(e.value)
    assert not os.path.exists(out)


def test_collate_keyword_is_checked(tmp_path):
    bam, gtf = lr.fixture_paths('loader_mixed')
    ann = loader.Annotation(gtf, 'locus', 'None')
    with pytest.raises(ValueError, match="collate must be 'none', 'host' or 'device'"):
        loader.load_alignment(bam, ann, collate='gpu')
    with pytest.raises(ValueError, match="collate must be 'none', 'host' or 'device'"):
        loader.load_alignment(bam, ann, loader='device', collate='sort')
    with pytest.raises(ValueError, match="needs loader='device'"):
        loader.load_alignment(bam, ann, collate='host')
    with pytest.raises(ValueError, match='run the two separately'):
        loader.load_alignment(bam, ann, loader='device', collate='host', rewrite='device', updated_sam=(str(tmp_path / 'o'), str(tmp_path / 't')))
    assert not os.listdir(str(tmp_path))
    want = loader.load_alignment(bam, ann)
    lr.assert_same_load(loader.load_alignment(bam, ann, collate='none'), want)
