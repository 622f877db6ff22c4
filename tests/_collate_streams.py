"""Record streams for `--collate` at the sizes a real BAM has, and the definition of tsem_bam_collate.h a second time, in numpy
(no GPU, no library): what tests/test_collate_streams_host.py and tests/test_gpu_collate_scale.py share.

    stream(group, name_len, extra, seed, lead=0, trail=0) -> (uint8 array, rec_off int64 [n + 1])   framed records, no per-record loop
    collate_np(data, rec_off) -> (collated bytes, order, n_names, out_off)                         THE DEFINITION, vectorised
    alignment_combos(rec_off, order, out_off) -> {(source & 3, destination & 3, length & 3)}       the paths of k_collate_gather
    STREAMS, get(name), reference(name)                                                             the named inputs, built once
    REFUSED, refused(name)                                                                          streams with three bad records

collate_np shares nothing with the C bodies: the names go into a padded matrix, np.unique finds the groups and their first records, a
stable argsort of those gives `order`.  tests/_collate_reference.py holds the written definition (a dict and a `sorted`) and the
inputs of a few hundred records; this file is for everything above one sort block.

The sizes sit on both sides of the limits at which rocprim::radix_sort_keys (default config, 8-byte keys) changes its algorithm
(rocprim/device/device_radix_sort.hpp, device_radix_sort_config.hpp):
    n <= block_size * items_per_thread of its single-block config = min(256, .) * min(4, .) = 1,024     one block sorts
    n <= radix_sort_config<>::merge_sort_limit = 1024 * 1024 = 1,048,576                                block sorts, then merges
    above                                                                                              Onesweep
"""
import functools
from collections import OrderedDict, namedtuple

import numpy as np

SINGLE_BLOCK_LIMIT = 256 * 4                       # rocprim: kernel_config<min(256, .), min(4, .)> of radix_sort_keys' single sort
MERGE_SORT_LIMIT = 1024 * 1024                     # rocprim: radix_sort_config<>::merge_sort_limit
WIDE_MEAN = 1024                                   # tsem_bam_collate: k_collate_gather<64> when total / n_rec >= 1024, else <16>
FIXED = 36                                         # block_size and the 32 fixed bytes: the name begins here
FILLER = 0x71                                      # the byte every name begins with; the groups differ in the last bytes
EDGE_N = (1, 2, 3, 63, 64, 65, 255, 256, 257)
LEAD_TRAIL = ((1, 0), (2, 1), (3, 2), (5, 3))

Stream = namedtuple('Stream', 'data off')
Reference = namedtuple('Reference', 'out order n_names out_off')


# ---- the streams ------------------------------------------------------------------------------------------------------
def _rank_in_class(cls):
    """for every element, how many earlier elements have the same value"""
    o = np.argsort(cls, kind='stable')
    s = cls[o]
    start = np.flatnonzero(np.r_[True, s[1:] != s[:-1]])
    rank = np.empty(len(cls), np.int64)
    rank[o] = np.arange(len(cls)) - np.repeat(start, np.diff(np.r_[start, len(cls)]))
    return rank


def stream(group, name_len, extra, seed, lead=0, trail=0):
    """Framed BAM records: record i has the name of group group[i] (name_len[g] bytes and the NUL; at most one group may have 0, the
    smallest record there is) and extra[i] bytes behind it.  block_size at 0, l_read_name at 12 and the name at 36 are what they must
    be; EVERY other byte is seeded random, the rest of the fixed fields too, so a copy that is off by one to three bytes cannot
    compare equal.  The name of a group is FILLER bytes and, in its last (up to 4) bytes, the group's number among the groups of its
    length in base 255 (no NUL inside): groups differ in their last bytes, or in their length.  `lead` random bytes lie in front
    (rec_off[0] = lead), `trail` behind rec_off[n]."""
    group, name_len, extra = np.asarray(group, np.int64), np.asarray(name_len, np.int64), np.asarray(extra, np.int64)
    n = len(group)
    assert len(extra) == n and name_len.min() >= 0 and name_len.max() <= 254 and extra.min() >= 0
    rank = _rank_in_class(name_len)
    room = np.where(name_len < 4, 255 ** np.minimum(name_len, 4), 255 ** 4)
    assert np.all(rank < room), 'more groups of one name length than names of that length'
    L = name_len[group]
    off = np.empty(n + 1, np.int64)
    off[0] = lead
    np.cumsum(FIXED + L + 1 + extra, out=off[1:])
    off[1:] += lead
    data = np.random.default_rng(seed).integers(0, 256, int(off[n]) + trail, dtype=np.uint8)
    at = off[:-1]
    size = (off[1:] - at - 4).astype('<u4')
    for b in range(4):
        data[at + b] = (size >> np.uint32(8 * b)).astype(np.uint8)
    data[at + 12] = L + 1
    for j in range(int(L.max()) if n else 0):                    # (a loop over the byte position, every record at once)
        m = L > j
        data[at[m] + FIXED + j] = FILLER
    for k in range(4):
        m = L > k
        digit = (rank // 255 ** k % 255 + 1).astype(np.uint8)
        data[at[m] + FIXED + L[m] - 1 - k] = digit[group[m]]
    data[at + FIXED + L] = 0
    return data, off


def group_first(data, rec_off):
    """-> (first int64 [n]: the first record of every record's group, the number of groups)"""
    data, off = np.frombuffer(data, np.uint8), np.asarray(rec_off, np.int64)
    n = len(off) - 1
    at, lens = off[:-1], np.diff(off)
    l = data[at + 12].astype(np.int64)
    assert lens.min() > FIXED and l.min() >= 1 and np.all(FIXED + l <= lens), 'the definition covers well-formed records only'
    names = np.zeros((n, 1 + int(l.max())), np.uint8)             # (l_read_name, the name, zeros)
    names[:, 0] = l
    for j in range(int(l.max())):                                 # (a loop over the byte position)
        m = l > j
        names[m, 1 + j] = data[at[m] + FIXED + j]
    rows = names.view(np.dtype((np.void, names.shape[1]))).ravel()
    _, index, inverse = np.unique(rows, return_index=True, return_inverse=True)
    return index[inverse.ravel()], len(index)


def collate_np(data, rec_off):
    """THE DEFINITION of tsem_bam_collate.h for a stream of records that bam_collate_check accepts: the groups of equal names
    (l_read_name and that many bytes at 36) in the order of their first records, inside a group the input order.
    -> (collated bytes, order, n_names, out_off int64 [n + 1])"""
    data, off = np.frombuffer(data, np.uint8), np.asarray(rec_off, np.int64)
    n = len(off) - 1
    if n == 0:
        return np.empty(0, np.uint8), np.empty(0, np.int64), 0, np.zeros(1, np.int64)
    at, lens = off[:-1], np.diff(off)
    first, n_names = group_first(data, off)
    order = np.argsort(first, kind='stable')
    out_off = np.zeros(n + 1, np.int64)
    np.cumsum(lens[order], out=out_off[1:])
    out = np.empty(int(out_off[n]), np.uint8)
    step = 1 << 16                                                # one fancy-index gather, in pieces that bound the index array
    for a in range(0, n, step):
        b = min(n, a + step)
        src = np.repeat(at[order[a:b]] - out_off[a:b], lens[order[a:b]]) + np.arange(out_off[a], out_off[b])
        out[out_off[a]:out_off[b]] = data[src]
    return out, order, n_names, out_off


def alignment_combos(rec_off, order, out_off):
    """the set of (source offset & 3, destination offset & 3, length & 3) over the output records: k_collate_gather's head, sh and
    tail, and whether it reads src[q + 1], are functions of these three"""
    off = np.asarray(rec_off, np.int64)
    s, ln = off[:-1][order], np.diff(off)[order]
    code = np.unique((s & 3) * 16 + (np.asarray(out_off, np.int64)[:-1] & 3) * 4 + (ln & 3))
    return {(int(c) >> 4, int(c) >> 2 & 3, int(c) & 3) for c in code}


def gather_width(rec_off):
    """the W of k_collate_gather<W> that tsem_bam_collate's host side selects"""
    n = len(rec_off) - 1
    return 64 if n and int(rec_off[n] - rec_off[0]) // n >= WIDE_MEAN else 16


def _name_lens(rng, groups, lo, hi):
    """name lengths lo .. hi, with no more groups of length 1 and 2 than there are such names"""
    ln = rng.integers(lo, hi + 1, groups)
    over = _rank_in_class(ln) >= np.where(ln < 3, 255 ** np.minimum(ln, 3), 1 << 62)
    ln[over] = rng.integers(max(lo, 3), hi + 1, int(over.sum()))
    return ln


def _small_groups(rng, n):
    """group numbers of n records in groups of 1 to 3, shuffled"""
    sizes = rng.integers(1, 4, n)
    g = np.repeat(np.arange(n), sizes)[:n]
    return rng.permutation(g)


def _pairs(rng, n):
    """two records per name, their positions a random permutation (a coordinate-sorted paired-end file); with n odd the LAST record
    is a group of its own, the only one whose `first` needs the top bit of a record index"""
    g = rng.permutation(np.repeat(np.arange(n // 2), 2))
    return np.r_[g, n // 2] if n & 1 else g


def _edge(n):
    """shuffled groups of 1 to 3 records; where n = 2^k + 1 the last record is a group of its own, as in _pairs"""
    rng = np.random.default_rng(100 + n)
    top = n > 2 and (n - 1) & (n - 2) == 0
    g = np.r_[_small_groups(rng, n - 1), n] if top else _small_groups(rng, n)
    return stream(g, _name_lens(rng, n + 1, 1, 40), rng.integers(0, 24, n), 200 + n)


def _paired(n, seed):
    rng = np.random.default_rng(seed)
    g = _pairs(rng, n)
    return stream(g, _name_lens(rng, int(g.max()) + 1, 1, 40), rng.integers(0, 24, n), seed + 1)


def _zipf(n, seed):
    """one group of 120,000 records scattered over the whole stream, the others of Zipf-distributed sizes 1 .. 64 (most of them singletons);
    the last record a group of its own"""
    rng = np.random.default_rng(seed)
    big, rest = 120000, n - 1 - 120000
    sizes = np.minimum(rng.zipf(1.6, rest), 64)
    sizes = sizes[:int(np.searchsorted(np.cumsum(sizes), rest)) + 1]
    g = np.r_[np.zeros(big, np.int64), 1 + np.repeat(np.arange(len(sizes)), sizes)[:rest]]
    g = np.r_[rng.permutation(g), int(g.max()) + 1]
    return stream(g, _name_lens(rng, int(g.max()) + 1, 1, 40), rng.integers(0, 24, n), seed + 1)


def _identity(kind, n, seed):
    """streams that are collated already: order is the identity, the output the input"""
    rng = np.random.default_rng(seed)
    if kind == 'one_name':
        g = np.zeros(n, np.int64)
    elif kind == 'all_distinct':
        g = np.arange(n)
    else:
        g = np.repeat(np.arange(n), rng.integers(1, 5, n))[:n]
    return stream(g, _name_lens(rng, int(g.max()) + 1, 1, 40), rng.integers(0, 24, n), seed + 1)


def _chains():
    """20,000 records over 4,096 names of every length: with 8 bits of the hash an average probe chain holds 16 names"""
    rng = np.random.default_rng(41)
    g = rng.permutation(np.r_[np.arange(4096), rng.integers(0, 4096, 20000 - 4096)])
    return stream(g, _name_lens(rng, 4096, 1, 254), rng.integers(0, 24, 20000), 42)


def _narrow(lead=0, trail=0, n=5000):
    rng = np.random.default_rng(51)
    g = _small_groups(rng, n)
    return stream(g, _name_lens(rng, n, 1, 40), rng.integers(0, 64, n), 52, lead=lead, trail=trail)


def _last_byte():
    """gather_narrow's records with the last of the l_read_name bytes, the NUL of a well-formed name, replaced by 0 or 1: names are
    compared as l_read_name bytes, so records that differ there alone are different names"""
    data, off = _narrow()
    at = off[:-1]
    data[at + FIXED + data[at + 12].astype(np.int64) - 1] = np.random.default_rng(53).integers(0, 2, len(at), dtype=np.uint8)
    return data, off


def _wide():
    """4,096 records: about 30 % of 37 .. 44 bytes (names of 0 .. 7 bytes), the others of 0.9 .. 2.4 KB, one of 70,001 bytes"""
    rng = np.random.default_rng(61)
    n, short_groups, long_groups = 4096, 40, 1500
    name_len = np.r_[0, rng.integers(1, 8, short_groups - 1), _name_lens(rng, long_groups, 8, 40)]
    small = rng.random(n) < 0.3
    small[:2] = (True, False)
    g = np.where(small, rng.integers(0, short_groups, n), short_groups + rng.integers(0, long_groups, n))
    g[0] = 0                                                      # the smallest record there is: 37 bytes
    L = name_len[g]
    extra = np.where(small, rng.integers(0, 8, n) % (8 - L.clip(max=7)), rng.integers(900, 2401, n) - FIXED - 1 - L)
    extra[0] = 0
    extra[1] = 70001 - FIXED - 1 - L[1]
    p = rng.permutation(n)
    return stream(g[p], name_len, extra[p], 62)


def _width(mean):
    """600 records whose framed lengths add up to 1024 * 600 (mean 1024) or to one byte less (mean 1023): the last input record's
    extra bytes make up the sum, every other record is the same in both"""
    rng = np.random.default_rng(71)
    n = 600
    g = np.r_[_small_groups(rng, n - 1), 0]                        # (the last record joins an early group: it lies inside the output)
    name_len = _name_lens(rng, n, 1, 40)
    extra = np.r_[rng.integers(800, 1101, n - 1), 0]
    extra[n - 1] = 1024 * n - int((FIXED + name_len[g] + 1 + extra).sum()) - (1024 - mean)
    assert extra[n - 1] > 0
    return stream(g, name_len, extra, 72)


def _spec(build, *hash_bits):
    return build, hash_bits or (0,)


STREAMS = OrderedDict()                                          # name -> (a function without arguments, the hash_bits it is run with)
for _n in EDGE_N:
    STREAMS['edge_n_%d' % _n] = _spec(functools.partial(_edge, _n))
STREAMS['single_block_1024'] = _spec(functools.partial(_paired, SINGLE_BLOCK_LIMIT, 300))
STREAMS['merge_1025'] = _spec(functools.partial(_paired, SINGLE_BLOCK_LIMIT + 1, 310))
STREAMS['merge_2p20'] = _spec(functools.partial(_paired, MERGE_SORT_LIMIT, 320))
STREAMS['onesweep_2p20p1'] = _spec(functools.partial(_paired, MERGE_SORT_LIMIT + 1, 330))
STREAMS['onesweep_zipf'] = _spec(functools.partial(_zipf, MERGE_SORT_LIMIT + 1, 340))
STREAMS['one_name_300001'] = _spec(functools.partial(_identity, 'one_name', 300001, 350))
STREAMS['all_distinct_300001'] = _spec(functools.partial(_identity, 'all_distinct', 300001, 360))
STREAMS['already_collated_300001'] = _spec(functools.partial(_identity, 'already_collated', 300001, 370))
STREAMS['chains_bits8'] = _spec(_chains, 8)
STREAMS['chains_bits12'] = _spec(_chains, 12)
STREAMS['gather_narrow'] = _spec(_narrow, 0, 4)
STREAMS['last_byte_5000'] = _spec(_last_byte, 0, 4)
STREAMS['gather_wide'] = _spec(_wide)
STREAMS['width_1023'] = _spec(functools.partial(_width, 1023))
STREAMS['width_1024'] = _spec(functools.partial(_width, 1024))
for _lead, _trail in LEAD_TRAIL:
    STREAMS['lead_trail_%d_%d' % (_lead, _trail)] = _spec(functools.partial(_narrow, _lead, _trail))

IDENTITY = ('one_name_300001', 'all_distinct_300001', 'already_collated_300001')
POW2_PLUS_1 = ('edge_n_3', 'edge_n_65', 'edge_n_257', 'merge_1025', 'onesweep_2p20p1', 'onesweep_zipf')
RUNS = [(name, bits) for name, (_build, all_bits) in STREAMS.items() for bits in all_bits]
RUN_IDS = ['%s-bits%d' % r for r in RUNS]


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=None)
def get(name):
    """-> Stream(data, off) of STREAMS[name], built once, read-only"""
    return Stream(*_frozen(*STREAMS[name][0]()))


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> Reference(out, order, n_names, out_off): collate_np of the stream, computed once, read-only"""
    out, order, names, out_off = collate_np(*get(name))
    return Reference(*_frozen(out, order), names, *_frozen(out_off))


# ---- several malformed records in one stream --------------------------------------------------------------------------
REFUSED_AT = (257, 2600, 4999)                                   # in the second, the eleventh and the last block of 256 lanes
REFUSED = ('short_first', 'noname_first', 'past_first')


@functools.lru_cache(maxsize=None)
def refused(name):
    """-> (data, off, the record that must be reported, its code): gather_narrow's 5,000 records with the three malformed kinds of
    _collate_reference.malformed() in the places REFUSED_AT, each kind once the earliest"""
    import _collate_reference as cr
    m = cr.malformed()
    kinds = [(m['shorter_than_33'][0][2], 1), (bytes(m['l_read_name_0'][0][1]), 2), (bytes(m['name_past_the_end'][0][0]), 3)]
    r = REFUSED.index(name)
    kinds = kinds[r:] + kinds[:r]
    data, off = get('gather_narrow')
    pieces, lens, at = [], np.diff(off), 0
    for i, (rec, _code) in zip(REFUSED_AT, kinds):
        pieces += [data[off[at]:off[i]], np.frombuffer(rec, np.uint8)]
        lens[i] = len(rec)
        at = i + 1
    pieces.append(data[off[at]:])
    new_off = np.r_[0, np.cumsum(lens)].astype(np.int64)
    out = np.concatenate(pieces)
    assert len(out) == new_off[-1]
    return _frozen(out, new_off) + (REFUSED_AT[0], kinds[0][1])


# ---- what a difference means ------------------------------------------------------------------------------------------
def describe_order(want, got, first):
    """the words of a failure whose `order` differs: where, and what is left of the properties of a collated order (`first`:
    group_first of the stream)"""
    want, got = np.asarray(want), np.asarray(got)
    n = len(want)
    k = int(np.flatnonzero(want != got)[0])
    perm = bool(np.array_equal(np.sort(got), np.arange(n)))
    text = 'first at output %d of %d (record %d, the definition has %d); still a permutation: %s' % (k, n, got[k], want[k], perm)
    if perm:
        grouped = 1 + np.count_nonzero(np.diff(first[got])) == len(np.unique(first))        # every group is one run
        text += '; still grouped: %s (%s)' % (grouped, "whole groups in the wrong order, or a group's records: `bits` or the sort's stability"
                                              if grouped else 'a group is torn: hash or insert')
    return text


def describe_bytes(rec_off, order, out_off, want, got):
    """the words of a failure whose order is right and whose bytes differ: the record, its path through the gather"""
    want, got = np.frombuffer(want, np.uint8), np.frombuffer(got, np.uint8)
    if len(want) != len(got):
        return 'the output has %d bytes, the definition %d' % (len(got), len(want))
    b = int(np.flatnonzero(want != got)[0])
    k = int(np.searchsorted(out_off, b, side='right')) - 1
    i = int(order[k])
    s, ln, d = int(rec_off[i]), int(rec_off[i + 1] - rec_off[i]), int(out_off[k])
    return ('first at byte %d = byte %d of output record %d (input record %d): (source & 3, destination & 3, length & 3) = (%d, %d, %d), '
            'length %d, W = %d' % (b, b - d, k, i, s & 3, d & 3, ln & 3, ln, gather_width(rec_off)))
