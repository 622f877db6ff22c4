"""The definition of `--collate` in plain Python, and the small inputs that the host and the GPU tests of it share (no GPU needed).

    collate(records) -> (records in collated order, order)       # the definition: a dict of first appearances and a `sorted`

`records` are framed (block_size and body).  cases() builds the streams that tsem_bam_collate_host and the kernels are held to;
reordered_files() writes the fixture and fuzz BAMs with their records sorted by (ref, pos) and shuffled, and each one's reference-collated
copy.  These inputs stay inside one block of the device's sort; tests/_collate_streams.py has the sizes above it (a vectorised
definition, held to collate() in tests/test_collate_streams_host.py).
"""
import os
import random
import struct
import subprocess
from collections import OrderedDict

import numpy as np

import _bam_fuzz as fuzz
import _loader_reference as lr
from telescope_amd import bam_out, loader

ROOT, CSRC, GOLD = lr.ROOT, lr.CSRC, lr.GOLD
HASH_BITS = (0, 1, 4)


def name_of(rec):
    """the name of a framed record: l_read_name bytes at offset 36, the NUL included"""
    return bytes(rec[36:36 + rec[12]])


def collate(records):
    """THE DEFINITION.  Groups of equal names in the order of their first records, inside a group the input order."""
    first = {}
    for i, r in enumerate(records):
        first.setdefault(name_of(r), i)
    order = sorted(range(len(records)), key=lambda i: (first[name_of(records[i])], i))
    return [records[i] for i in order], order


def frame(body):
    return struct.pack('<i', len(body)) + body


def stream_of(records):
    """-> (bytes, rec_off int64 [n + 1]) of framed records"""
    off = np.zeros(len(records) + 1, np.int64)
    if records:
        off[1:] = np.cumsum([len(r) for r in records])
    return b''.join(records), off


def split(data, off):
    return [bytes(data[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


def _rec(name, pos=100, n=20, **kw):
    return frame(fuzz.encode(name, 0, 0, pos, [(n, 'M')], AS=-1, **kw))


def smallest_record(name=b''):
    """32 fixed bytes and the name's NUL: no CIGAR, no sequence, no aux"""
    return frame(struct.pack('<iiBBHHHiiii', -1, -1, len(name) + 1, 0, 4680, 0, 4, 0, -1, -1, 0) + name + b'\x00')


def cases():
    """name -> framed records; every situation the issue lists"""
    rng = random.Random(20)
    c = OrderedDict()
    c['n0'] = []
    c['n1'] = [_rec('only')]
    c['one_name'] = [_rec('same', pos=10 * k, n=5 + k % 7) for k in range(70)]
    c['all_distinct'] = [_rec('d%04d' % k, n=1 + k % 9) for k in range(300)]
    c['already_collated'] = [_rec('g%03d' % g, pos=k) for g in range(60) for k in range(1 + g % 4)]
    c['name_lengths_1_254'] = [_rec('a'), _rec('b' * 254), _rec('c'), _rec('b' * 254, pos=7), _rec('a', pos=9), _rec('b' * 253 + 'c')]
    pre = ['r1', 'r10', 'r1' + 'x' * 250, 'r', 'r100']
    c['prefixes'] = [_rec(pre[k % 5], pos=k) for k in rng.sample(range(40), 40)]
    c['last_byte_differs'] = [_rec('q' * 30 + 'abcd'[rng.randrange(4)], pos=k) for k in range(80)]
    mixed = [_rec('solo')] + [_rec('big', pos=k, n=1 + k % 5) for k in range(200)] + [_rec('mid%d' % (k % 7), pos=k) for k in range(50)]
    rng.shuffle(mixed)
    c['groups_of_1_and_200'] = mixed
    c['first_and_last'] = [_rec('ends')] + [_rec('m%d' % (k % 11), pos=k) for k in range(90)] + [_rec('ends', pos=5)]
    c['sizes_mod_4'] = [_rec('s' * (1 + k % 4) + '%d' % (k % 3), pos=k, n=k % 8) for k in rng.sample(range(64), 64)]
    c['smallest'] = [smallest_record(), _rec('z'), smallest_record(b'y'), smallest_record(), _rec('z', pos=3), smallest_record(b'y')]
    c['above_128k'] = [_rec('long', pos=1), _rec('short'), _rec('long', pos=2, n=140000), _rec('short', pos=4), _rec('long', pos=3, n=3000)]
    return c


def malformed():
    """label -> (framed records, the record that must be refused, its code)"""
    good = _rec('fine')
    short = frame(struct.pack('<iiBBHHHiiii', 0, 1, 1, 0, 0, 0, 0, 0, -1, -1, 0))                    # 32 bytes: no room for a name
    noname = bytearray(_rec('x')); noname[12] = 0
    past = bytearray(smallest_record(b'abc')); past[12] = 5                                         # 4 name bytes, l_read_name 5
    return OrderedDict([('shorter_than_33', ([good, good, short, good], 2, 1)), ('l_read_name_0', ([good, bytes(noname)], 1, 2)),
                        ('name_past_the_end', ([bytes(past), good], 0, 3))])


# ---- the fixture and fuzz BAMs, reordered -----------------------------------------------------------------------------
FIXTURES = ('bundled', 'loader_mixed', 'sc_mixed')
FUZZ_SEEDS = (0, 1, 2)


def _header(path):
    return loader.read_bam(path, raw=True)[2]


def write_bam(path, header, framed):
    with bam_out.BamWriter(path, header) as w:
        w.write_framed(b''.join(framed))


def _sort_key(rec):
    ref, pos = struct.unpack_from('<ii', rec, 4)
    return (ref if ref >= 0 else 1 << 31, pos)                 # (unmapped records last, as a coordinate sort puts them)


def reordered(records, how, seed=0):
    if how == 'sorted':
        return sorted(records, key=_sort_key)
    out = list(records)
    random.Random(1000 + seed).shuffle(out)
    return out


def sources(directory):
    """[(label, bam, gtf, barcode tag)] of the three fixtures and the three fuzz cases"""
    out = []
    for name in FIXTURES:
        bam, gtf = lr.fixture_paths(name)
        out.append((name, bam, gtf, lr.FIXTURES[name][0]))
    for seed in FUZZ_SEEDS:
        case = fuzz.make_case(seed, directory)
        out.append(('fuzz%d' % seed, case.bam, case.gtf, None))
    return out


def reordered_files(directory, source, how):
    """-> (the reordered BAM, its reference-collated copy, the reordered framed records) of one of sources()"""
    label, bam, _gtf, _tag = source
    _refs, data, off = lr.inflated_records(bam)
    recs = reordered(split(data, off), how, seed=len(label))
    header = _header(bam)
    p_in = os.path.join(directory, '%s-%s.bam' % (label, how))
    p_ref = os.path.join(directory, '%s-%s-collated.bam' % (label, how))
    write_bam(p_in, header, recs)
    write_bam(p_ref, header, collate(recs)[0])
    return p_in, p_ref, recs


# ---- the stand-alone program ------------------------------------------------------------------------------------------
def build_host_program(directory, sanitize=True):
    """tests/c_host/bam_collate_check.cc as an ordinary host program (its own main), with the address and undefined-behaviour sanitizers"""
    exe = os.path.join(directory, 'bam_collate_check')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-Wno-unknown-pragmas', '-I' + CSRC, os.path.join(ROOT, 'tests', 'c_host', 'bam_collate_check.cc'),
           '-o', exe]
    if sanitize:
        cmd[1:1] = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer']
    subprocess.run(cmd, check=True)
    return exe


def host_run(exe, records, hash_bits, directory, tag='case'):
    """-> (collated bytes, order, names), or (code, record) for a refused input; a sanitizer report fails it"""
    src, dst = os.path.join(directory, tag + '.in'), os.path.join(directory, tag + '.out')
    with open(src, 'wb') as fh:
        fh.write(struct.pack('<q', len(records)))
        for r in records:
            fh.write(struct.pack('<q', len(r)) + r)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    p = subprocess.run([exe, src, dst, str(hash_bits)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert p.returncode == 0 and not p.stderr, 'bam_collate_check failed (%d):\n%s' % (p.returncode, p.stderr.decode()[-4000:])
    words = p.stdout.decode().split()
    if words[0] == 'refused':
        return int(words[1]), int(words[2])
    assert words[0] == 'names'
    raw = open(dst, 'rb').read()
    n = len(records)
    order = np.frombuffer(raw, np.int64, n).tolist()
    return raw[8 * n:], order, int(words[1])
