"""Run container for the `telescope resume` path: checkpoint I/O, RNG seed, reports.

Mirrors the caller contract of the reference's `Telescope` class
(/root/reference/telescope/utils/model.py:74-564) as far as the accelerated
path needs it: `load` / `save` (model.py:108-148, the `.npz` checkpoint schema),
`get_random_seed` (model.py:150-153), `print_summary` (model.py:523-555) and
`output_report` (model.py:420-477, the two TSVs incl. the header glued to the
RunInfo comment), and, with `--updated_sam`, the two BAMs of the load and `update_sam` (model.py:479-521).
"""
import logging as lg
from collections import Counter, OrderedDict

import numpy as np
import pandas as pd
import scipy.sparse as sp


def _str2int(s):
    """helpers.py:149-156 — run_info values come back as int, float or str."""
    for cast in (int, float):
        try:
            return cast(s)
        except ValueError:
            pass
    return s


class NpzSlices(object):
    """Parts of the arrays of an `.npz` without reading the file: `np.savez` (model.py:133) stores its members UNCOMPRESSED, so
    element [a, b) of a 1-D member sits at a known offset of the archive — the local zip header, then the `.npy` header, then the
    raw values — and is read with one seek + readinto.  A compressed member (np.savez_compressed) is read whole, once, and sliced."""

    def __init__(self, filename):
        import zipfile
        self.filename = filename
        self._zf = zipfile.ZipFile(filename)
        self._whole = {}

    def close(self):
        self._zf.close()

    def names(self):
        return [n[:-4] for n in self._zf.namelist() if n.endswith('.npy')]

    def _member(self, name):
        import struct
        import zipfile
        info = self._zf.getinfo(name + '.npy')
        if info.compress_type != zipfile.ZIP_STORED:
            return None
        with open(self.filename, 'rb') as fh:
            fh.seek(info.header_offset)
            hdr = fh.read(30)                                   # local file header: signature, ..., name length (26), extra length (28)
            if hdr[:4] != b'PK\x03\x04':
                return None
            n_name, n_extra = struct.unpack('<HH', hdr[26:30])
            fh.seek(info.header_offset + 30 + n_name + n_extra)
            major, _minor = np.lib.format.read_magic(fh)
            shape, fortran, dtype = (np.lib.format.read_array_header_1_0(fh) if major == 1 else np.lib.format.read_array_header_2_0(fh))
            return fh.tell(), shape, fortran, dtype

    def shape(self, name):
        m = self._member(name)
        return m[1] if m is not None else self.whole(name).shape

    def whole(self, name):
        if name not in self._whole:
            with self._zf.open(name + '.npy') as fh:
                self._whole[name] = np.lib.format.read_array(fh, allow_pickle=False)
        return self._whole[name]

    def read(self, name, start=0, stop=None):
        """Elements [start, stop) of the 1-D member `name` (a fresh array)."""
        m = self._member(name)
        if m is None or len(m[1]) != 1 or m[3].hasobject:
            a = self.whole(name)
            return np.array(a[start:stop])
        off, shape, _fortran, dtype = m
        stop = shape[0] if stop is None else min(stop, shape[0])
        start = min(max(start, 0), stop)
        out = np.empty(stop - start, dtype=dtype)
        with open(self.filename, 'rb') as fh:
            fh.seek(off + start * dtype.itemsize)
            got = fh.readinto(memoryview(out).cast('B')) if out.size else 0
        if got != out.nbytes:
            raise IOError('%s: member %s is shorter than its header says' % (self.filename, name))
        return out


def write_bootstrap_tsv(fh, names, count, fits, level=0.95):
    """One comment line — replicates, seed, fitted, converged, method, level — then per locus, sorted by name like TE_counts.tsv:
    `count` (the point estimate, as TE_counts.tsv prints it), mean / sd / lower / upper bound of the bootstrap counts (2 decimals)
    and of the bootstrap final_prop (%.6g), over the fitted replicates (`BootstrapFits.summary`)."""
    s = fits.summary(level)
    cols = OrderedDict([('transcript', list(names)), ('count', np.asarray(count))])
    for key, pre, fmt in (('counts', 'count', '%.2f'), ('pi', 'prop', '%.6g')):
        for stat in ('mean', 'sd', 'lo', 'hi'):
            cols['%s_%s' % (pre, stat)] = [fmt % v for v in s[key][stat]]
    table = pd.DataFrame(cols)
    table.sort_values('transcript', inplace=True)
    fh.write('\t'.join(['## Bootstrap', 'replicates:%d' % fits.n_rep, 'seed:%d' % fits.seed, 'fitted:%d' % int(fits.fitted.sum()),
                        'converged:%d' % int(fits.converged.sum()), 'method:%s' % fits.method, 'level:%g' % level]) + '\n')
    table.to_csv(fh, sep='\t', index=False)


class Telescope(object):
    def __init__(self, opts=None):
        self.opts = opts
        self.run_info = OrderedDict()
        self.feature_length = Counter()
        self.read_index, self.feat_index = {}, {}
        self.shape = None
        self.raw_scores = None
        self.row_range = None            # (r0, r1): `raw_scores` holds only these fragments (load_shard); None = all of them

    # ---- alignment loading (model.py:155-173, via telescope_amd/loader.py) --------
    @property
    def other_bam(self):
        return self.opts.outfile_path('other.bam')               # model.py:89-92

    @property
    def tmp_bam(self):
        return self.opts.outfile_path('tmp_tele.bam')

    def _updated_sam_paths(self):
        return (self.other_bam, self.tmp_bam) if getattr(self.opts, 'updated_sam', False) else None

    def load_alignment(self, annotation):
        from . import loader
        o = self.opts
        self.run_info['annotated_features'] = len(annotation.loci)
        r = loader.load_alignment(o.samfile, annotation, o.no_feature_key, o.overlap_mode,
                                  o.overlap_threshold, o.stranded_mode, updated_sam=self._updated_sam_paths(),
                                  loader=getattr(o, 'loader', 'python'), device=getattr(o, 'device', 0), inflate=getattr(o, 'inflate', 'host'),
                                  rewrite=getattr(o, 'rewrite', 'host'), deflate=getattr(o, 'deflate', 'host'), collate=getattr(o, 'collate', 'none'))
        self._take_tmp_table()
        self.feature_length = r['feature_length']
        self.read_index, self.feat_index = r['read_index'], r['feat_index']
        self.raw_scores = r['raw_scores']
        self.shape = self.raw_scores.shape
        for k, v in r['run_info'].items():
            self.run_info[k] = v

    # ---- checkpoint (model.py:108-148) -------------------------------------
    def save(self, filename):
        feats = sorted(self.feat_index, key=self.feat_index.get)
        raw = sp.csr_matrix(self.raw_scores)
        np.savez(filename,
                 _run_info=list(self.run_info.items()),
                 _flen_list=[self.feature_length[f] for f in feats],
                 _feat_list=feats,
                 _read_list=sorted(self.read_index, key=self.read_index.get),
                 _shape=self.shape,
                 _raw_scores_data=raw.data, _raw_scores_indices=raw.indices,
                 _raw_scores_indptr=raw.indptr, _raw_scores_shape=raw.shape)

    @classmethod
    def load(cls, filename):
        z = np.load(filename)
        obj = cls()
        for k, v in z['_run_info']:
            obj.run_info[str(k)] = _str2int(str(v))
        for f, fl in zip(z['_feat_list'], z['_flen_list']):
            obj.feature_length[str(f)] = fl
        obj.read_index = {str(n): i for i, n in enumerate(z['_read_list'])}
        obj.feat_index = {str(n): i for i, n in enumerate(z['_feat_list'])}
        obj.shape = (len(obj.read_index), len(obj.feat_index))
        if tuple(z['_shape']) != obj.shape:
            raise AssertionError('checkpoint shape %s does not match its name lists %s'
                                 % (tuple(z['_shape']), obj.shape))
        obj.raw_scores = sp.csr_matrix((z['_raw_scores_data'], z['_raw_scores_indices'],
                                        z['_raw_scores_indptr']), shape=tuple(z['_raw_scores_shape']))
        return obj

    @classmethod
    def load_shard(cls, filename, world, rank):
        """This rank's share of a checkpoint for a row-sharded run: the run information, the feature lists and the row pointers are
        read whole (K- and N-sized), the stored entries only for the rank's contiguous range of fragments — balanced by entries,
        `distributed.shard_bounds` — straight from their offsets in the archive (NpzSlices), and the fragment names (`_read_list`,
        the largest member after the entries; nothing on the EM / report path uses them) not at all.  A rank of an 8-way run of the
        50M-fragment checkpoint touches 1.6 GB of a 12.4 GB file instead of all of it.  `raw_scores` is the rank's (r1 - r0) x K
        slice, `row_range` = (r0, r1), `shape` the whole matrix's (the seed rule uses it, model.py:150-153)."""
        from .distributed import shard_bounds
        z = NpzSlices(filename)
        try:
            obj = cls()
            for k, v in z.whole('_run_info'):
                obj.run_info[str(k)] = _str2int(str(v))
            feats, flens = z.whole('_feat_list'), z.whole('_flen_list')
            for f, fl in zip(feats, flens):
                obj.feature_length[str(f)] = fl
            obj.feat_index = {str(n): i for i, n in enumerate(feats)}
            obj.read_index = None                                # not loaded (see above)
            obj.shape = tuple(int(x) for x in z.whole('_shape'))
            n_rows, n_cols = (int(x) for x in z.whole('_raw_scores_shape'))
            if obj.shape != (n_rows, n_cols) or len(obj.feat_index) != n_cols or z.shape('_read_list')[0] != n_rows:
                raise AssertionError('checkpoint shape %s does not match its matrix %s / name lists' % (obj.shape, (n_rows, n_cols)))
            indptr = z.read('_raw_scores_indptr')
            r0, r1 = shard_bounds(n_rows, world, rank, indptr=indptr)
            e0, e1 = int(indptr[r0]), int(indptr[r1])
            local_ptr = indptr[r0:r1 + 1] - indptr[r0]
            del indptr
            obj.raw_scores = sp.csr_matrix((z.read('_raw_scores_data', e0, e1), z.read('_raw_scores_indices', e0, e1), local_ptr),
                                           shape=(r1 - r0, n_cols))
            obj.row_range = (r0, r1)
            return obj
        finally:
            z.close()

    def get_random_seed(self):
        """model.py:150-153 — note the precedence: (total % N) * K, then mod 2^32-1."""
        ret = self.run_info['total_fragments'] % self.shape[0] * self.shape[1]
        return ret % 4294967295

    # ---- log summary (model.py:523-555) -----------------------------------------
    def print_summary(self, loglev=lg.WARNING):
        d = Counter()
        for k, v in self.run_info.items():
            try:
                d[k] = int(v)
            except ValueError:
                pass
        if 'mapped_pairs' in d:
            d['pair_mapped'] = d['mapped_pairs']
        if 'mapped_single' in d:
            d['single_mapped'] = d['mapped_single']
        say = lambda m: lg.log(loglev, m)  # noqa: E731
        say("Alignment Summary:")
        say('    {} total fragments.'.format(d['total_fragments']))
        say('        {} mapped as pairs.'.format(d['pair_mapped']))
        say('        {} mapped as mixed.'.format(d['pair_mixed']))
        say('        {} mapped single.'.format(d['single_mapped']))
        say('        {} failed to map.'.format(d['unmapped']))
        say('--')
        say('    {} fragments mapped to reference; of these'.format(
            d['pair_mapped'] + d['pair_mixed'] + d['single_mapped']))
        say('        {} had one unique alignment.'.format(d['unique']))
        say('        {} had multiple alignments.'.format(d['ambig']))
        say('--')
        say('    {} fragments overlapped annotation; of these'.format(d['overlap_unique'] + d['overlap_ambig']))
        say('        {} map to one locus.'.format(d['overlap_unique']))
        say('        {} map to multiple loci.'.format(d['overlap_ambig']))
        say('\n')

    # ---- reports (model.py:420-477) -----------------------------------------------
    def output_report(self, tl, stats_filename, counts_filename, write=True):
        """Same columns, evaluation order (the RNG is consumed by init_best_random before the
        final mode), sort, rounding and file layout as the reference — including the header row
        glued onto the RunInfo comment line (model.py:470-471 writes no newline)."""
        mode, prob = self.opts.reassign_mode, self.opts.conf_prob
        names = sorted(self.feat_index, key=self.feat_index.get)
        colsum = getattr(tl, 'reassign_colsums', None) or \
            (lambda m, t=0.9, initial=False: tl.reassign(m, t, initial).sum(0).A1)
        stats = pd.DataFrame(OrderedDict([
            ('transcript', names),
            ('transcript_length', [self.feature_length[f] for f in names]),
            ('final_conf', colsum('conf', prob)),
            ('final_prop', tl.pi),
            ('init_aligned', colsum('all', initial=True)),
            ('unique_count', colsum('unique')),
            ('init_best', colsum('exclude', initial=True)),
            ('init_best_random', colsum('choose', initial=True)),
            ('init_best_avg', colsum('average', initial=True)),
            ('init_prop', tl.pi_init),
        ]))
        stats.sort_values('final_prop', ascending=False, inplace=True)
        stats = stats.round(pd.Series([2, 3, 2, 3],
                                      index=['final_conf', 'final_prop', 'init_best_avg', 'init_prop']))
        counts = pd.DataFrame(OrderedDict([('transcript', names), ('count', colsum(mode, prob))]))
        counts.sort_values('transcript', inplace=True)
        if not write:                                        # a rank other than 0 of a row-sharded run: it took part in the sums
            return
        comment = ['## RunInfo'] + ['{}:{}'.format(k, v) for k, v in self.run_info.items()]
        with open(stats_filename, 'w') as fh:
            fh.write('\t'.join(comment))
            stats.to_csv(fh, sep='\t', index=False)
        with open(counts_filename, 'w') as fh:
            counts.to_csv(fh, sep='\t', index=False)

    def output_bootstrap(self, tl, fits, filename, level=0.95):
        """`<exp_tag>-bootstrap.tsv` of `--bootstrap N`: per locus the count of TE_counts.tsv and the bootstrap statistics of that
        count and of final_prop (write_bootstrap_tsv)."""
        mode, prob = self.opts.reassign_mode, self.opts.conf_prob
        names = sorted(self.feat_index, key=self.feat_index.get)
        colsum = getattr(tl, 'reassign_colsums', None) or \
            (lambda m, t=0.9, initial=False: tl.reassign(m, t, initial).sum(0).A1)
        with open(filename, 'w') as fh:
            write_bootstrap_tsv(fh, names, colsum(mode, prob), fits, level)

    # ---- updated alignment file (model.py:479-521) ---------------------------------------------------------------------------
    def update_sam(self, tl, filename, command_line=None):
        """model.py:479-521: the tmp BAM of the load, re-read fragment by fragment (the reference's bundling and pairing), written to
        `filename` with the input's header plus one @PG line.  Unmapped pairs unchanged; a SEC pair gets flag 0x100, MAPQ 0 and
        YC 248,248,248; a PRI pair MAPQ phred(z), XP int(round(z * 100)) and — assigned by reassign(reassign_mode, conf_prob) —
        0x100 cleared and YC vermilion, else 0x100 set and YC yellow (z >= 0.2) or GPAL[2]; z = tl.z[row, ZF's column] (0 outside
        z's pattern).  The tags come from the device (tsem_entry_tags) in tiles of consecutive rows: fragment rows rise in the tmp
        BAM's order, so the tiles are visited once, in order; a name that comes back in a later bundle (an input that is not
        collated) maps to an earlier row, whose tags are asked again for that one row.  `choose` draws its picks ONCE here, after
        the report's draws, like the reference's fresh `tl.reassign` (model.py:483).  Single GPU: row-sharded runs are refused."""
        import sys
        from . import bam_out, loader
        if getattr(tl, 'comm', None) is not None and tl.comm.world > 1:
            raise NotImplementedError('update_sam: row-sharded runs (WORLD_SIZE > 1) are not supported')
        mode, prob = self.opts.reassign_mode, self.opts.conf_prob
        asg = tl.reassign(mode, prob)                            # (choose: the draw happens here, as in the reference)
        raw = sp.csr_matrix(self.raw_scores)
        indptr, indices = raw.indptr, raw.indices
        if getattr(self, 'tmp_table', None) is not None:         # --rewrite device: the load left what every tmp record needs
            return self._update_sam_device(tl, filename, command_line, asg, indptr, indices, raw.shape[1])
        tiles = tl.entry_tag_tiles(mode, prob, assignment=asg)
        cur = (0, 0, None)                                       # the tile in hand: rows [r0, r1), their words
        back = {}                                                # rows met again behind the tile in hand

        def word(ridx, fidx):
            nonlocal cur
            r0, r1, w = cur
            if ridx >= r1:
                for cur in tiles:
                    if ridx < cur[1]:
                        break
                r0, r1, w = cur
                if not r0 <= ridx < r1:
                    raise AssertionError('update_sam: row %d outside the matrix' % ridx)
                base = indptr[r0]
            elif ridx < r0:
                if ridx not in back:
                    back[ridx] = tl.entry_tags(ridx, ridx + 1, mode, prob, assignment=asg)
                w, base = back[ridx], indptr[ridx]
            else:
                base = indptr[r0]
            s, e = indptr[ridx], indptr[ridx + 1]
            k = s + int(np.searchsorted(indices[s:e], fidx))
            return int(w[k - base]) if k < e and indices[k] == fidx else 0

        _, records, header = loader.read_bam(self.tmp_bam, raw=True)
        text = bam_out.header_with_pg(header['text'], self.run_info.get('version', getattr(self.opts, 'version', '')),
                                      ' '.join(sys.argv) if command_line is None else command_line)
        deflate = getattr(self.opts, 'deflate', 'host')
        try:
            with bam_out.BamWriter(filename, header, text, deflate=deflate, device=getattr(self.opts, 'device', 0)) as out:
                for _code, pairs in loader._fragments(records):
                    if not pairs:
                        continue
                    ridx = self.read_index[pairs[0].r1.qname]
                    for p in pairs:
                        recs = p.records()
                        if p.is_unmapped:
                            for r in recs:
                                out.write(r)
                            continue
                        zt = bam_out.get_tag(recs[0], 'ZT')
                        if zt is None:
                            raise AssertionError('Missing ZT tag')
                        w = 0
                        if zt != 'SEC':
                            w = word(ridx, self.feat_index[bam_out.get_tag(recs[0], 'ZF')])
                        for r in bam_out.update_pair(recs, zt, w):
                            out.write(r)
            self._log_device_deflate(out)
        finally:
            tiles.close()

    @staticmethod
    def _log_device_deflate(out):
        """one line after a BamWriter with deflate='device' is closed: the blocks and batches that went through the device"""
        from . import bam_out
        if out is not None and out.deflate == 'device':
            st = bam_out.sum_device_stats([out])
            lg.info('device deflate: %d BGZF blocks of updated in %d batches' % (st['deflate_blocks'], st['deflate_batches']))
            return st
        return None

    def _take_tmp_table(self):
        """after a load: the device loader's table of the tmp BAM's records (`--rewrite device`), None otherwise"""
        self.tmp_table = None
        if getattr(self.opts, 'rewrite', 'host') == 'device':
            from . import loader_device
            self.tmp_table = loader_device.LAST_TMP_TABLE

    UPDATE_CHUNK_BYTES = 64 << 20
    LAST_UPDATE_STATS = {}

    def _update_sam_device(self, tl, filename, command_line, asg, indptr, indices, n_cols):
        """update_sam with the records rewritten on the GPU (tsem_bam_update_size / tsem_bam_rewrite_fetch): the same file, byte for
        byte.  The load's table says per tmp record the kind, the row and the column; the tag words of the PRI records are looked up
        with numpy against the CSR, tile by tile of tl.entry_tag_tiles; the tmp BAM is read in chunks (gzip, or the device inflate
        under --inflate device), every chunk's records are walked again on the device, rewritten and handed to the BGZF writer.  No
        per-record Python."""
        import gzip
        import io
        import sys
        from time import perf_counter
        from . import bam_out, loader
        from ._lib import BAM_STATUS, BamLoader, EngineError, bam_scan
        t_all = perf_counter()
        stats = dict(records=0, chunks=0, bytes=0, lookup_s=0., read_s=0., device_s=0., deflate_s=0.)
        mode, prob = self.opts.reassign_mode, self.opts.conf_prob
        tab = self.tmp_table
        kind, row, col = tab['kind'], tab['row'].astype(np.int64), tab['col'].astype(np.int64)
        words = kind.astype(np.uint32) << np.uint32(30)
        t0 = perf_counter()
        pri = np.flatnonzero(kind == 2)
        tiles = tl.entry_tag_tiles(mode, prob, assignment=asg)
        try:
            if pri.size:
                if row[pri].min() < 0 or row[pri].max() >= len(indptr) - 1:
                    raise AssertionError('update_sam: a row outside the matrix')
                key_e = np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(indptr)) * n_cols + indices
                key_q = row[pri] * n_cols + col[pri]
                pos = np.searchsorted(key_e, key_q)
                ok = pos < key_e.size
                ok[ok] = key_e[pos[ok]] == key_q[ok]
                pos = np.where(ok, pos, -1)                      # the entry of (row, column), -1: not stored -> word 0
                del key_e, key_q
                for r0, r1, w in tiles:
                    m = (pos >= indptr[r0]) & (pos < indptr[r1])
                    words[pri[m]] |= np.asarray(w, dtype=np.uint32)[pos[m] - indptr[r0]]
        finally:
            tiles.close()
        stats['lookup_s'] = perf_counter() - t0
        device = getattr(self.opts, 'device', 0)
        if getattr(self.opts, 'inflate', 'host') == 'device':
            from .bgzf import DeviceBgzfReader
            fh = DeviceBgzfReader(self.tmp_bam, device=device)
        else:
            fh = io.BufferedReader(gzip.open(self.tmp_bam, 'rb'), buffer_size=1 << 20)
        dev = out = None
        z = np.zeros(0, np.int64)
        try:
            _refs, text, block = loader.read_bam_header(fh, self.tmp_bam)
            header = dict(text=text.split(b'\x00', 1)[0].decode(), refs_block=block)
            text = bam_out.header_with_pg(header['text'], self.run_info.get('version', getattr(self.opts, 'version', '')),
                                          ' '.join(sys.argv) if command_line is None else command_line)
            out = bam_out.BamWriter(filename, header, text, deflate=getattr(self.opts, 'deflate', 'host'), device=device)
            dev = BamLoader(device, z, z, z, z, z, z, z)
            done, tail = 0, b''
            while True:
                t0 = perf_counter()
                new = fh.read(self.UPDATE_CHUNK_BYTES)
                data = tail + new if tail else new
                try:
                    off, used = bam_scan(data)
                except EngineError as e:
                    raise ValueError('%s: behind record %d: %s' % (self.tmp_bam, done, e))
                n = len(off) - 1
                t1 = perf_counter()
                stats['read_s'] += t1 - t0
                if done + n > len(words):
                    raise ValueError('%s holds more records than the %d the load wrote' % (self.tmp_bam, len(words)))
                if n:
                    pos, (st, rec) = dev.update_size(data[:used], off, words[done:done + n])
                    if st:
                        o = int(off[rec])
                        name = bytes(data[o + 36:min(o + 35 + data[o + 12], int(off[rec + 1]))]).decode(errors='replace')
                        raise ValueError('%s: record %d (%s): %s' % (self.tmp_bam, done + rec, name, BAM_STATUS.get(st, 'status %d' % st)))
                    _, stream = dev.rewrite_fetch(0, pos[n])
                    t2 = perf_counter()
                    stats['device_s'] += t2 - t1
                    out.write_framed(stream)
                    stats['deflate_s'] += perf_counter() - t2
                    stats['bytes'] += int(pos[n])
                done += n; stats['chunks'] += 1
                tail = data[used:]
                if not new:
                    break
            if tail:
                raise ValueError('%s: truncated BAM record behind record %d' % (self.tmp_bam, done))
            if done != len(words):
                raise ValueError('%s holds %d records, the load wrote %d' % (self.tmp_bam, done, len(words)))
            stats['records'] = done
            stats['kernels_ms'] = dev.rewrite_times()
        finally:
            fh.close()
            if dev is not None:
                dev.close()
            if out is not None:
                t0 = perf_counter()
                out.close()
                stats['deflate_s'] += perf_counter() - t0
        st = self._log_device_deflate(out)
        if st:
            stats.update(st, deflate='device')
        stats['total_s'] = perf_counter() - t_all
        Telescope.LAST_UPDATE_STATS = stats


# ---- single-cell mode (scTelescope, model.py:567-629) -----------------------------------------------------------------------------
SC_METHODS = ('conf', 'all', 'unique', 'exclude', 'choose', 'average')   # model.py:618: the order fixes when `choose` draws


def _float_repr(v):
    return repr(float(v))


def write_dense_counts(fh, csr, barcodes, features, block=None):
    """`pd.DataFrame(csr.todense(), columns=features, index=barcodes).to_csv(fh, sep='\t')` (model.py:626-629), byte for byte, streamed
    from the CSR: no dense array is built — a line starts as K copies of `0.0` and only the stored entries are formatted (repr, as
    pandas writes float64: `3.0`, `0.3333333333333333`).  Lines go out in blocks of `block` cells (default: ~32 MB of text each)."""
    csr = sp.csr_matrix(csr)
    csr.sort_indices()
    n_cells, k = csr.shape
    if len(barcodes) != n_cells or len(features) != k:
        raise ValueError('write_dense_counts: %d barcodes / %d features for a %s matrix' % (len(barcodes), len(features), csr.shape))
    if block is None:
        block = max(1, (32 << 20) // (4 * max(k, 1)))
    fh.write('\t'.join([''] + [_csv_field(f) for f in features]) + '\n')
    zeros = ['0.0'] * k
    ip, ix, dv = csr.indptr, csr.indices, csr.data
    for c0 in range(0, n_cells, block):
        out = []
        for c in range(c0, min(n_cells, c0 + block)):
            vals = list(zeros)
            for j, v in zip(ix[ip[c]:ip[c + 1]].tolist(), dv[ip[c]:ip[c + 1]].tolist()):
                vals[j] = repr(v)
            out.append(_csv_field(barcodes[c]) + '\t' + '\t'.join(vals) + '\n')
        fh.write(''.join(out))


def _csv_field(s):
    """a field as pandas' csv writer quotes it with sep='\\t' (QUOTE_MINIMAL)"""
    s = str(s)
    if any(ch in s for ch in ('\t', '"', '\n', '\r')):
        return '"' + s.replace('"', '""') + '"'
    return s


def write_mtx_counts(mtx_path, csr, barcodes, features):
    """Matrix Market (cells x features, real general, full precision) at `mtx_path`; `<stem>-barcodes.tsv` and `<stem>-features.tsv`
    beside it (one name per line), where <stem> is the path up to `-TE_counts`."""
    import scipy.io
    scipy.io.mmwrite(mtx_path, sp.coo_matrix(csr), field='real', precision=17)
    cut = mtx_path.rfind('-TE_counts')
    stem = mtx_path[:cut] if cut >= 0 else mtx_path[:mtx_path.rfind('.')]
    for suffix, names in (('-barcodes.tsv', barcodes), ('-features.tsv', features)):
        with open(stem + suffix, 'w') as fh:
            fh.writelines('%s\n' % n for n in names)


def read_celltype_tsv(path):
    """`--celltype_tsv`: tab-separated `barcode<TAB>celltype` lines, no header; empty lines and lines starting with `#` are skipped.
    Returns {barcode: type name} in file order.  ValueError: the file cannot be read, a line without two fields, a barcode listed with
    two different types."""
    out = OrderedDict()
    try:
        with open(path) as fh:
            lines = fh.read().splitlines()
    except (OSError, UnicodeDecodeError) as e:
        raise ValueError('cannot read %s: %s' % (path, e))
    for no, line in enumerate(lines, 1):
        if not line.strip() or line.startswith('#'):
            continue
        f = line.split('\t')
        if len(f) != 2 or not f[0].strip() or not f[1].strip():
            raise ValueError('%s, line %d: expected barcode<TAB>celltype, got %r' % (path, no, line))
        bc, name = f[0].strip(), f[1].strip()
        if out.setdefault(bc, name) != name:
            raise ValueError('%s, line %d: barcode %s is listed with two cell types (%s, %s)' % (path, no, bc, out[bc], name))
    return out


def celltype_map(barcodes, type_of_barcode):
    """The types numbered in sorted order of their names, and the type of every cell of the run (-1: a barcode the file does not
    list; barcodes of the file that the run does not contain are ignored).  ValueError when the file names no barcode of the run."""
    names = sorted(set(type_of_barcode.values()))
    number = {n: i for i, n in enumerate(names)}
    type_of_cell = np.asarray([number[type_of_barcode[b]] if b in type_of_barcode else -1 for b in barcodes], dtype=np.int32)
    if not np.any(type_of_cell >= 0):
        raise ValueError('the cell type file names none of the %d barcodes of this run' % len(barcodes))
    return names, type_of_cell


def compose_type_of_row(cell_of_row, type_of_cell):
    """type_of_cell[cell_of_row], -1 for a fragment without barcode or of a barcode without type"""
    cor = np.asarray(cell_of_row)
    out = np.full(cor.shape, -1, np.int32)
    has = cor >= 0
    out[has] = np.asarray(type_of_cell, dtype=np.int32)[cor[has]]
    return out


class scTelescope(Telescope):
    """Single-cell run container: the bulk container plus the cell of every fragment (`cell_of_row`, -1 = no barcode) and the cell
    names in first-appearance order (`barcodes`) — what the reference keeps as `barcode_read_indices` (model.py:311-316)."""

    def __init__(self, opts=None):
        super().__init__(opts)
        self.cell_of_row = None
        self.barcodes = []
        self.type_names, self.type_of_cell = None, None      # `--pooling_mode celltype` (set_celltypes)
        self.umi_of_row, self.umis = None, None              # `--umi_tag`: the UMI of every fragment (-1 = none), the distinct values
        self.umi_dedup = None                                # the UmiDedup of collapse_umis
        self._umi_frags = None                               # per barcode, before the collapse: fragments, fragments with a UMI

    def set_celltypes(self, type_of_barcode):
        """The cell types of `--celltype_tsv` (read_celltype_tsv) for this run's barcodes; ValueError if it names none of them."""
        self.type_names, self.type_of_cell = celltype_map(self.barcodes, type_of_barcode)

    def load_alignment(self, annotation):
        from . import loader
        o = self.opts
        self.run_info['annotated_features'] = len(annotation.loci)
        r = loader.load_alignment(o.samfile, annotation, o.no_feature_key, o.overlap_mode, o.overlap_threshold, o.stranded_mode,
                                  barcode_tag=o.barcode_tag, updated_sam=self._updated_sam_paths(), umi_tag=getattr(o, 'umi_tag', None),
                                  loader=getattr(o, 'loader', 'python'), device=getattr(o, 'device', 0), inflate=getattr(o, 'inflate', 'host'),
                                  rewrite=getattr(o, 'rewrite', 'host'), deflate=getattr(o, 'deflate', 'host'), collate=getattr(o, 'collate', 'none'))
        self._take_tmp_table()
        self.feature_length = r['feature_length']
        self.read_index, self.feat_index = r['read_index'], r['feat_index']
        self.raw_scores = r['raw_scores']
        self.shape = self.raw_scores.shape
        for k, v in r['run_info'].items():
            self.run_info[k] = v
        self.cell_of_row, self.barcodes = r['cell_of_row'], r['barcodes']
        if 'umi_of_row' in r:
            self.umi_of_row, self.umis = r['umi_of_row'], r['umis']

    def save(self, filename):
        """The bulk checkpoint's keys, byte for byte, plus `_barcode_list` (unicode, cell order) and `_read_barcode` (int32 per row,
        -1 = none) and, only when UMIs were read (`--umi_tag`), `_umi_list` and `_read_umi` likewise.  The bulk `load` and the
        reference's `Telescope.load` read named keys only and ignore them."""
        feats = sorted(self.feat_index, key=self.feat_index.get)
        raw = sp.csr_matrix(self.raw_scores)
        more = {}
        if self.umi_of_row is not None:
            more = dict(_umi_list=np.array(list(self.umis), dtype=np.str_), _read_umi=np.asarray(self.umi_of_row, dtype=np.int32))
        np.savez(filename,
                 _run_info=list(self.run_info.items()),
                 _flen_list=[self.feature_length[f] for f in feats],
                 _feat_list=feats,
                 _read_list=sorted(self.read_index, key=self.read_index.get),
                 _shape=self.shape,
                 _raw_scores_data=raw.data, _raw_scores_indices=raw.indices,
                 _raw_scores_indptr=raw.indptr, _raw_scores_shape=raw.shape,
                 _barcode_list=np.array(list(self.barcodes), dtype=np.str_),
                 _read_barcode=np.asarray(self.cell_of_row, dtype=np.int32), **more)

    @classmethod
    def load(cls, filename):
        obj = super(scTelescope, cls).load(filename)
        z = np.load(filename)
        if '_barcode_list' not in z.files or '_read_barcode' not in z.files:
            raise ValueError('%s is not a single-cell checkpoint (no _barcode_list / _read_barcode): write one with '
                             '`sc assign`' % filename)
        obj.barcodes = [str(b) for b in z['_barcode_list']]
        obj.cell_of_row = np.asarray(z['_read_barcode'], dtype=np.int32)
        if obj.cell_of_row.shape != (obj.shape[0],) or (obj.cell_of_row.size and obj.cell_of_row.max() >= len(obj.barcodes)):
            raise ValueError('%s: _read_barcode does not match the matrix / _barcode_list' % filename)
        if '_umi_list' in z.files or '_read_umi' in z.files:
            if '_umi_list' not in z.files or '_read_umi' not in z.files:
                raise ValueError('%s: _umi_list and _read_umi come together' % filename)
            obj.umis = [str(u) for u in z['_umi_list']]
            obj.umi_of_row = np.asarray(z['_read_umi'], dtype=np.int32)
            if obj.umi_of_row.shape != (obj.shape[0],) or (obj.umi_of_row.size and (obj.umi_of_row.max() >= len(obj.umis) or
                                                                                    obj.umi_of_row.min() < -1)):
                raise ValueError('%s: _read_umi does not match the matrix / _umi_list' % filename)
        return obj

    def collapse_umis(self, device=0):
        """Collapse the UMI duplicates (likelihood.umi_dedup): `raw_scores`, `shape`, `cell_of_row`, `umi_of_row` and `read_index`
        become those of the kept fragments, renumbered in order; K and the feature list stay.  The `UmiDedup` (row numbers of the
        uncollapsed run) is kept as `self.umi_dedup` and returned."""
        from .likelihood import umi_dedup
        if self.umi_of_row is None:
            raise ValueError('collapse_umis: no UMIs were read (load the alignments with --umi_tag)')
        d = umi_dedup(self.raw_scores, self.cell_of_row, self.umi_of_row, device=device, n_cells=len(self.barcodes), n_umis=len(self.umis))
        cor, uor = np.asarray(self.cell_of_row), np.asarray(self.umi_of_row)
        n_cells = len(self.barcodes)
        self._umi_frags = (np.bincount(cor[cor >= 0], minlength=n_cells), np.bincount(cor[(cor >= 0) & (uor >= 0)], minlength=n_cells))
        keep = d.keep
        self.raw_scores = sp.csr_matrix(self.raw_scores)[np.flatnonzero(keep)]
        self.shape = self.raw_scores.shape
        self.cell_of_row, self.umi_of_row = cor[keep].astype(np.int32), uor[keep].astype(np.int32)
        if self.read_index is not None:
            new = np.cumsum(keep) - 1
            self.read_index = {name: int(new[i]) for name, i in self.read_index.items() if keep[i]}
        self.umi_dedup = d
        return d

    def write_umi_stats(self, filename):
        """`<exp_tag>-umi_stats.tsv` of a collapsed run: one line per barcode — its fragments, how many of them carry a UMI, and
        the fragments kept."""
        if self.umi_dedup is None:
            raise ValueError('write_umi_stats: the run is not collapsed (collapse_umis)')
        frags, with_umi = self._umi_frags
        kept = self.umi_dedup.kept_per_cell(len(self.barcodes))
        with open(filename, 'w') as fh:
            fh.write('barcode\tfragments\twith_umi\tkept\n')
            for c, b in enumerate(self.barcodes):
                fh.write('%s\t%d\t%d\t%d\n' % (_csv_field(b), frags[c], with_umi[c], kept[c]))

    def output_report(self, tl, stats_filename, counts_filename, write=True):
        """model.py:575-629: the stats TSV (transcript, transcript_length, final_prop, init_prop; sorted by final_prop, rounded; the
        RunInfo line ENDS with a newline here) and one per-cell count matrix per method asked — `--reassign_mode`, or all six with
        `--use_every_reassign_mode` (`<exp_tag>-TE_counts_<method>.tsv`, in the order conf, all, unique, exclude, choose, average).
        The matrices are built sparse on the device (reassign_cell_counts) and written streamed (tsv) or as Matrix Market (mtx)."""
        mode, prob = self.opts.reassign_mode, self.opts.conf_prob
        every = bool(getattr(self.opts, 'use_every_reassign_mode', False))
        fmt = getattr(self.opts, 'count_format', 'tsv')
        names = sorted(self.feat_index, key=self.feat_index.get)
        stats = pd.DataFrame(OrderedDict([
            ('transcript', names),
            ('transcript_length', [self.feature_length[f] for f in names]),
            ('final_prop', tl.pi),
            ('init_prop', tl.pi_init),
        ]))
        stats.sort_values('final_prop', ascending=False, inplace=True)
        stats = stats.round(pd.Series([2, 3, 2, 3], index=['final_conf', 'final_prop', 'init_best_avg', 'init_prop']))
        if write:
            comment = ['## RunInfo'] + ['{}:{}'.format(k, v) for k, v in self.run_info.items()]
            with open(stats_filename, 'w') as fh:
                fh.write('\t'.join(comment) + '\n')
                stats.to_csv(fh, sep='\t', index=False)
        n_cells = len(self.barcodes)
        pooling = getattr(self.opts, 'pooling_mode', 'pseudobulk')
        count_map = self.cell_of_row
        if pooling == 'individual':
            # one model per cell: from here on tl's z is the per-cell posteriors, and the counts below come from them
            fits = tl.em_cells(self.cell_of_row, n_cells, bool(getattr(self.opts, 'use_likelihood', False)), loglev=lg.INFO)
            if write:
                self.write_cell_stats(tl, fits, stats_filename.replace('run_stats.tsv', 'cell_stats.tsv')
                                      if stats_filename.endswith('run_stats.tsv') else stats_filename + '.cell_stats.tsv')
        elif pooling == 'celltype':
            # one model per cell type: every cell's counts come from the posteriors of its type's fit; a barcode without type is
            # in no group, gets no posterior and counts nowhere
            if self.type_of_cell is None:
                self.set_celltypes(self.opts.celltypes)
            type_of_row = compose_type_of_row(self.cell_of_row, self.type_of_cell)
            lost = np.asarray(self.cell_of_row) >= 0
            lost &= type_of_row < 0
            if lost.any():
                lg.warning('%d barcodes (%d fragments) have no cell type in %s: their counts are zero'
                           % (int(np.sum(self.type_of_cell < 0)), int(lost.sum()), getattr(self.opts, 'celltype_tsv', 'the cell type file')))
            fits = tl.em_cells(type_of_row, len(self.type_names), bool(getattr(self.opts, 'use_likelihood', False)), loglev=lg.INFO)
            if write:
                self.write_celltype_stats(tl, fits, stats_filename.replace('run_stats.tsv', 'celltype_stats.tsv')
                                          if stats_filename.endswith('run_stats.tsv') else stats_filename + '.celltype_stats.tsv')
            count_map = np.where(type_of_row >= 0, np.asarray(self.cell_of_row), -1).astype(np.int32)
        for method in SC_METHODS:
            if method != mode and not every:
                continue
            out = counts_filename[:counts_filename.rfind('.')] + '_' + method + '.tsv' if every else counts_filename
            counts = tl.reassign_cell_counts(method, count_map, n_cells, prob)
            if not write:
                continue
            if fmt == 'mtx':
                write_mtx_counts(out[:out.rfind('.')] + '.mtx', counts, self.barcodes, names)
            else:
                with open(out, 'w') as fh:
                    write_dense_counts(fh, counts, self.barcodes, names)

    def output_cell_bootstrap(self, fits, mean_filename, sd_filename):
        """`<exp_tag>-TE_counts_boot_mean` / `_boot_sd` of a single-cell run's bootstrap (`tl.bootstrap(..., cell_of_row=self.cell_of_row)`): mean and standard deviation (ddof 1) of every
        barcode's count over the good replicates (`fits.cells`, a BootstrapCells), in the layout and by the writers of the count
        matrix itself — dense tsv or Matrix Market, per `--count_format` (the file names are given with `.tsv`)."""
        fmt = getattr(self.opts, 'count_format', 'tsv')
        names = sorted(self.feat_index, key=self.feat_index.get)
        for out, matrix in ((mean_filename, fits.cells.mean_matrix()), (sd_filename, fits.cells.sd_matrix())):
            if fmt == 'mtx':
                write_mtx_counts(out[:out.rfind('.')] + '.mtx', matrix, self.barcodes, names)
            else:
                with open(out, 'w') as fh:
                    write_dense_counts(fh, matrix, self.barcodes, names)

    def write_cell_stats(self, tl, fits, filename):
        """`<exp_tag>-cell_stats.tsv` of `--pooling_mode individual`: one line per barcode — its fragments, how many of them are
        ambiguous, the features it touches, and its fit's iterations, convergence and log-likelihood."""
        cor = np.asarray(self.cell_of_row)
        n_cells = len(self.barcodes)
        in_cell = cor >= 0
        frags = np.bincount(cor[in_cell], minlength=n_cells)
        amb = np.bincount(cor[in_cell], weights=np.asarray(tl.Y).ravel()[in_cell], minlength=n_cells).astype(np.int64)
        with open(filename, 'w') as fh:
            fh.write('barcode\tfragments\tambiguous\tcolumns\titerations\tconverged\tlnl\n')
            for c in range(n_cells):
                fh.write('%s\t%d\t%d\t%d\t%d\t%s\t%s\n' % (_csv_field(self.barcodes[c]), frags[c], amb[c],
                                                            fits.col_ptr[c + 1] - fits.col_ptr[c], fits.n_iter[c],
                                                            bool(fits.converged[c]), _float_repr(fits.lnl[c])))

    def write_celltype_stats(self, tl, fits, filename):
        """`<exp_tag>-celltype_stats.tsv` of `--pooling_mode celltype`: one line per type — its cells, its fragments, how many of
        them are ambiguous, the features it touches, and its fit's iterations, convergence and log-likelihood."""
        n_types = len(self.type_names)
        toc = np.asarray(self.type_of_cell)
        tor = compose_type_of_row(self.cell_of_row, toc)
        in_type = tor >= 0
        cells = np.bincount(toc[toc >= 0], minlength=n_types)
        frags = np.bincount(tor[in_type], minlength=n_types)
        amb = np.bincount(tor[in_type], weights=np.asarray(tl.Y).ravel()[in_type], minlength=n_types).astype(np.int64)
        with open(filename, 'w') as fh:
            fh.write('celltype\tcells\tfragments\tambiguous\tcolumns\titerations\tconverged\tlnl\n')
            for t in range(n_types):
                fh.write('%s\t%d\t%d\t%d\t%d\t%d\t%s\t%s\n' % (_csv_field(self.type_names[t]), cells[t], frags[t], amb[t],
                                                                 fits.col_ptr[t + 1] - fits.col_ptr[t], fits.n_iter[t],
                                                                 bool(fits.converged[t]), _float_repr(fits.lnl[t])))
