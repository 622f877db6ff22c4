"""Cases and expectations for the record rewriting of `--updated_sam` on the device (telescope_amd/csrc/tsem_bam_edit.h), shared by
the host test (the sanitized stand-alone program tests/c_host/bam_edit_check.cc) and the GPU tests.  What a rewritten record must
be is always said by telescope_amd/bam_out.py: set_tag / set_flag / set_mapq / update_pair on the record's raw bytes."""
import os
import struct
import subprocess

from telescope_amd import bam_out

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'telescope_amd', 'csrc')
KEEP, SEC, PRI = 0, 1, 2
NAMES = ('ZF', 'ZT', 'ZB', 'XP', 'YC')


def record(name='r', flag=0, aux=b'', mapq=30, ref=0, pos=100, cigar=((20, 0),), nref=-1, npos=-1, tlen=0):
    """one record's bytes (no block size); cigar: (length, op code) pairs; aux: the encoded aux fields"""
    l_seq = sum(n for n, op in cigar if op in (0, 1, 4, 7, 8))
    body = struct.pack('<iiBBHHHiiii', ref, pos, len(name) + 1, mapq, 0, len(cigar), flag, l_seq, nref, npos, tlen)
    body += name.encode() + b'\x00' + b''.join(struct.pack('<I', (n << 4) | op) for n, op in cigar)
    return body + bytes((l_seq + 1) // 2) + bytes([30]) * l_seq + aux


def aux_as(name, typ):
    """the aux field `name` with some value of type `typ` (Z A C i f B)"""
    n = name.encode()
    return {'Z': n + b'Zold value\x00', 'A': n + b'Aq', 'C': n + b'C\x07', 'i': n + b'i' + struct.pack('<i', -70000),
            'f': n + b'f' + struct.pack('<f', 2.5), 'B': n + b'BS' + struct.pack('<iHHH', 3, 1, 2, 3)}[typ]


OTHERS = (b'ASc\xfb', b'NMC\x01', b'XSZhello\x00', b'XBBc' + struct.pack('<ibb', 2, -1, 1))


def built_aux():
    """[(label, aux bytes)]: the smallest aux lists that can go wrong, see the test's docstring"""
    out = [('no aux at all', b'')]
    for nm in NAMES:
        out.append(('only %s' % nm, aux_as(nm, 'Z')))
        for typ in 'ZACifB':
            t = aux_as(nm, typ)
            out.append(('%s:%s first' % (nm, typ), t + OTHERS[0] + OTHERS[1]))
            out.append(('%s:%s middle' % (nm, typ), OTHERS[0] + t + OTHERS[2]))
            out.append(('%s:%s last' % (nm, typ), OTHERS[0] + OTHERS[3] + t))
        out.append(('%s twice' % nm, aux_as(nm, 'Z') + OTHERS[0] + aux_as(nm, 'i')))
        out.append(('%s twice in a row, last' % nm, OTHERS[1] + aux_as(nm, 'C') + aux_as(nm, 'B')))
    out.append(('all five, mixed', b''.join(aux_as(nm, typ) + OTHERS[k % 4] for k, (nm, typ) in enumerate(zip(NAMES, 'BZiAf')))))
    return out


def frame(rec):
    return struct.pack('<i', len(rec)) + rec


def word(kind, mapq=0, xp=0, assigned=False, high=False):
    return (kind << 30) | mapq | (xp << 8) | (int(assigned) << 16) | (int(high) << 17)


def updated(rec, w):
    """bam_out's answer for one record of a pair with word w"""
    kind = w >> 30
    if kind == KEEP:
        return rec
    return bam_out.update_pair([rec], 'SEC' if kind == SEC else 'PRI', w & 0x3ffff)[0]


def loaded(rec, zf, pri, zb):
    rec = bam_out.set_tag(rec, 'ZF', zf)
    rec = bam_out.set_tag(rec, 'ZT', 'PRI' if pri else 'SEC')
    return bam_out.set_tag(rec, 'ZB', zb)


def case_edit(rec, flag_and, flag_or, mapq, strip, append):
    assert len(strip) <= 4
    s = [n.encode()[0] | (n.encode()[1] << 8) for n in strip] + [0] * (4 - len(strip))
    return (struct.pack('<iq', 0, len(rec) + 4) + frame(rec) + struct.pack('<IIii4Hq', flag_and, flag_or, mapq, len(strip), *s, len(append))
            + append)


def case_update(rec, w):
    return struct.pack('<iq', 1, len(rec) + 4) + frame(rec) + struct.pack('<I', w)


def case_load(rec, names, feat, pri, mfeat, mas):
    """names: the locus names by id, the no_feature_key last; feat / mfeat: locus ids, -1 = no feature"""
    enc = [n.encode() for n in names]
    off = [0]
    for e in enc:
        off.append(off[-1] + len(e))
    return (struct.pack('<iq', 2, len(rec) + 4) + frame(rec) + struct.pack('<i%dq' % len(off), len(enc), *off) + b''.join(enc)
            + struct.pack('<iii', feat, int(pri), len(mfeat)) + struct.pack('<%di' % len(mfeat), *mfeat) + struct.pack('<%di' % len(mas), *mas))


def zb_of(names, mfeat, mas):
    return ','.join(names[f] for f, a in zip(mfeat, mas) if a == mas[0])


def build_host_program(directory, sanitize=True):
    """tests/c_host/bam_edit_check.cc as an ordinary host program (its own main), with the address and undefined-behaviour sanitizers"""
    exe = os.path.join(directory, 'bam_edit_check')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-Wno-unknown-pragmas', '-I' + CSRC, os.path.join(ROOT, 'tests', 'c_host', 'bam_edit_check.cc'),
           '-o', exe]
    if sanitize:
        cmd[1:1] = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer']
    subprocess.run(cmd, check=True)
    return exe


def host_load(exe, bam, ann, stranded_mode, no_feature_key, record_cap, directory, tag='load'):
    """The load stage of a whole BAM as one chunk in the host program, the bundles it leaves to the host spliced in with
    loader_device.host_bundle as load_alignment_device does -> (other stream, tmp stream, bundles left to the host)"""
    import _loader_reference as lr
    from telescope_amd import loader, loader_device as ld
    refs, data, off = lr.inflated_records(bam)
    p = lambda s: os.path.join(directory, tag + s)
    open(p('.rec'), 'wb').write(data)
    lr.write_annotation(ann, refs, p('.ann'))
    enc = [n.encode() for n in list(ann.loci) + [no_feature_key]]
    noff = [0]
    for e in enc:
        noff.append(noff[-1] + len(e))
    open(p('.names'), 'wb').write(struct.pack('<i%dq' % len(noff), len(enc), *noff) + b''.join(enc))
    cmd = [exe, '--load', p('.rec'), p('.ann'), p('.names'), str(int(ann.run_stranded)), str(int(stranded_mode[0] == 'F')),
           str(int(stranded_mode[-1] == 'F')), '0.2', str(record_cap), p('.other'), p('.tmp')]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert r.returncode == 0 and not r.stderr, 'bam_edit_check --load failed (%d):\n%s' % (r.returncode, r.stderr.decode()[-4000:])
    lines = r.stdout.decode().splitlines()
    assert lines[0] == 'status 0', lines[0]
    bundles = [tuple(int(x) for x in l.split()[1:]) for l in lines[1:]]
    streams = [open(p('.other'), 'rb').read(), open(p('.tmp'), 'rb').read()]
    assign = lambda pair: loader.assign_pair(pair, ann, refs, stranded_mode, no_feature_key, 0.2)
    out, at, hosted = [[], []], [0, 0], 0
    for k, (s, cls, po, pt) in enumerate(bundles):
        if cls != 5:
            continue
        hosted += 1
        e = bundles[k + 1][0] if k + 1 < len(bundles) else len(off) - 1
        h = ld.host_bundle(data, off, s, e, None, None, assign, no_feature_key, streams=True)
        for j, (pos, piece) in enumerate(((po, h['other']), (pt, h['tmp']))):
            out[j] += [streams[j][at[j]:pos], piece]; at[j] = pos
    return b''.join(out[0] + [streams[0][at[0]:]]), b''.join(out[1] + [streams[1][at[1]:]]), hosted


def record_stream(path):
    """the inflated bytes of a BAM file behind its header"""
    import gzip
    import io
    from telescope_amd import loader
    with gzip.open(path, 'rb') as g:
        raw = g.read()
    fh = io.BytesIO(raw)
    loader.read_bam_header(fh, path)
    return raw[fh.tell():]


def host_run(exe, cases, directory, tag='cases'):
    """-> per case the rewritten record's bytes (no block size; the block size is checked here), or -code; a sanitizer report fails it"""
    src, dst = os.path.join(directory, tag + '.in'), os.path.join(directory, tag + '.out')
    with open(src, 'wb') as fh:
        fh.write(b''.join(cases))
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    p = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert p.returncode == 0 and not p.stderr, 'bam_edit_check failed (%d):\n%s' % (p.returncode, p.stderr.decode()[-4000:])
    assert p.stdout.decode().split() == ['cases', str(len(cases))]
    raw = open(dst, 'rb').read()
    out, o = [], 0
    for _ in cases:
        (n,) = struct.unpack_from('<q', raw, o)
        o += 8
        if n < 0:
            out.append(int(n))
            continue
        assert struct.unpack_from('<i', raw, o)[0] == n - 4
        out.append(raw[o + 4:o + n]); o += n
    assert o == len(raw)
    return out
