"""ctypes binding of libtelescope_em.so (C ABI: include/telescope_em.h).

There is NO CPU fallback.  If the shared library is missing, or no HIP device
is usable, every entry point raises — the product path never computes on the
host.
"""
import ctypes as C
import itertools
import os
import sys
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# TSEM_LIB: kernel experiments (A/B builds of the same source); the product always uses the in-tree build
LIB_PATH = os.environ.get('TSEM_LIB') or os.path.join(HERE, 'libtelescope_em.so')

OK, ERR_ARG, ERR_HIP, ERR_NOMEM, ERR_TIMEOUT = 0, -1, -2, -3, -4
RA_CODE = {'exclude': 0, 'choose': 1, 'average': 2, 'conf': 3, 'unique': 4, 'all': 5}
Z_PREV, Z_CUR, Z_INITIAL, Z_FIRST, Z_USER = 0, 1, 2, 3, 4
EMK_AUTO, EMK_TWOPASS, EMK_FUSED = 0, 1, 2
# the cells of the fused kernel's table in the order of the launch census (fz_census_cell, csrc/tsem_index.h): team size, mode, entry
# format, geometry, timeline, index format; tests/test_fused_cells_host.py ties the order to the library's
FUSED_CELLS = tuple(itertools.product(range(1, 9), range(10), range(3), range(4), (0, 1), range(3)))


class EngineError(RuntimeError):
    code = 0


# host / ABI, set-up, EM support, report / row passes, collectives, CSR primitives, per-cell counts, per-cell fits, bootstrap,
# UMI duplicates, device loader, BGZF inflate, collate (telescope_amd/csrc/tsem_internal.h)
LIB_UNITS = ('tsem_host', 'tsem_setup', 'tsem_em', 'tsem_report', 'tsem_comm', 'tsem_csr', 'tsem_cells', 'tsem_cellem', 'tsem_boot',
             'tsem_umi', 'tsem_bam', 'tsem_bgzf', 'tsem_bam_collate')
FZ_UNITS = tuple('tsem_fz_p%d' % p for p in range(1, 9))


def build_library(force=False, verbose=False, out=None):
    """Compile the HIP library for gfx950 in-tree (hipcc cross-compiles without a GPU).  Twenty-one translation units — the thirteen of
    LIB_UNITS and the eight that instantiate the fused kernel for one team size each (most of the build time) — are compiled
    in parallel and linked into one shared object."""
    from concurrent.futures import ThreadPoolExecutor
    csrc = os.path.join(HERE, 'csrc')
    units = [os.path.join(csrc, u + '.hip') for u in LIB_UNITS + FZ_UNITS]
    deps = units + sorted(os.path.join(csrc, h) for h in os.listdir(csrc) if h.endswith('.h')) + [os.path.join(ROOT, 'include', 'telescope_em.h')]
    target = out or LIB_PATH
    objdir = os.path.join(csrc, '_obj' + ('' if out is None else '_' + os.path.basename(out)))
    common = ['hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-munsafe-fp-atomics', '-ffp-contract=off',
              '-I' + os.path.join(ROOT, 'include'), '-I' + csrc]
    link_stamp = os.path.join(objdir, '_link.flags')        # (a change of the compile flags alone must rebuild too)

    def unit_flags(src):
        # -ffp-contract=off everywhere but in the units of the persistent EM / lnl kernel.  The report, mask and z kernels must round
        # every product Q * (pi theta) before they add (the reference's sequence: the INTEGER outputs hang on exact ties between z
        # values; an FMA-contracted row sum was one ulp off and broke a tie in the sharded soak, tests/fuzz_reports.py seed 10).  The
        # fused kernel's sums feed pi / theta / lnl only (floating-point tolerance, their order of additions differs from scipy's
        # anyway), and its log-table lnl pass with fp64 entries spills 28 registers without contraction (4.6 -> 6.0 ms).
        return [f for f in common if f != '-ffp-contract=off'] if os.path.basename(src).startswith('tsem_fz_p') else common

    def stamp_ok(src):
        st = os.path.join(objdir, os.path.splitext(os.path.basename(src))[0] + '.o.flags')
        return os.path.exists(st) and open(st).read() == ' '.join(unit_flags(src))
    same_flags = os.path.exists(link_stamp) and open(link_stamp).read() == ' '.join(common) and all(stamp_ok(u) for u in units)
    if (not force and same_flags and os.path.exists(target) and all(os.path.getmtime(target) >= os.path.getmtime(d) for d in deps)):
        if verbose:
            print('build_library: %s is newer than all %d sources and headers: nothing to compile' % (os.path.relpath(target, ROOT), len(deps)),
                  flush=True)
        return target
    os.makedirs(objdir, exist_ok=True)

    import re

    def includes(path, seen):
        """Quoted #include closure of one source file (the library's own headers)."""
        for name in re.findall(r'^\s*#include\s+"([^"]+)"', open(path).read(), re.M):
            for d in (os.path.dirname(path), csrc, os.path.join(ROOT, 'include')):
                q = os.path.join(d, name)
                if os.path.exists(q) and q not in seen:
                    seen.add(q)
                    includes(q, seen)
        return seen

    def compile_unit(src):
        obj = os.path.join(objdir, os.path.splitext(os.path.basename(src))[0] + '.o')
        stamp = obj + '.flags'
        cu = unit_flags(src)
        flags = ' '.join(cu)
        if not force and os.path.exists(obj) and os.path.exists(stamp) and open(stamp).read() == flags and \
                all(os.path.getmtime(obj) >= os.path.getmtime(d) for d in [src] + sorted(includes(src, set()))):
            if verbose:
                print('up to date: %s' % os.path.relpath(obj, ROOT), flush=True)
            return obj                                   # this unit's object is newer than everything it is made from
        cmd = cu + ['-c', src, '-o', obj]
        if verbose:
            print(' '.join(cmd), flush=True)
        subprocess.run(cmd, check=True)
        open(stamp, 'w').write(flags)
        compiled.append(os.path.basename(src))
        return obj
    compiled = []
    with ThreadPoolExecutor(max_workers=len(units)) as ex:
        objs = list(ex.map(compile_unit, units))
    link = ['hipcc', '--offload-arch=gfx950', '-shared', '-fPIC', '-o', target] + objs + ['-ldl', '-lpthread']   # (RCCL is resolved at run time)
    if verbose:
        print(' '.join(link), flush=True)
    subprocess.run(link, check=True)
    with open(link_stamp, 'w') as fh:
        fh.write(' '.join(common))
    if verbose:      # what this call actually did (whether build() compiled anything must be visible)
        print('build_library: compiled %d of %d units (%s), linked %s' % (len(compiled), len(units), ', '.join(compiled) or 'none',
                                                                          os.path.relpath(target, ROOT)), flush=True)
    return target


def sources_fingerprint():
    """sha256 (16 hex digits) over the library's sources — what a measurement kept under profiles/ is stamped with, so that a later
    run can tell whether the kernels it describes are still the ones in the tree (bench.py `roofline.traffic_unit`)."""
    import hashlib
    csrc = os.path.join(HERE, 'csrc')
    names = sorted(f for f in os.listdir(csrc) if f.endswith(('.hip', '.h')))
    hsh = hashlib.sha256()
    for f in names + [os.path.join(ROOT, 'include', 'telescope_em.h')]:
        with open(f if os.path.isabs(f) else os.path.join(csrc, f), 'rb') as fh:
            hsh.update(fh.read())
    return hsh.hexdigest()[:16]


_lib = None


def _p(dtype):
    return np.ctypeslib.ndpointer(dtype=dtype, flags='C_CONTIGUOUS')


def exported_symbols():
    """Names the header declares; tests check the .so exports every one."""
    import re
    hdr = open(os.path.join(ROOT, 'include', 'telescope_em.h')).read()
    return sorted(set(re.findall(r'\b(tsem_[a-z0-9_]+)\s*\(', hdr)))


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EngineError(
            'libtelescope_em.so is not built (%s). Run `python -c "import __graft_entry__ as g; '
            'g.build()"`. There is no CPU fallback.' % LIB_PATH)
    # torch ships its own libamdhip64; if it is going to be used in this process (multi-GPU
    # plumbing), it must be loaded BEFORE ours so both share one HIP runtime.
    # A single-process command-line run never touches torch: TSEM_NO_TORCH=1 (set by telescope_amd/cli.py when it is not a rank
    # of a torch.distributed launch) saves the 1.5-2 s of `import torch` there.
    if 'torch' in sys.modules or os.environ.get('TSEM_NO_TORCH', '0') != '1':
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, u64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_double
    L.tsem_create.argtypes = [C.POINTER(vp), C.c_int]
    L.tsem_destroy.argtypes = [vp]
    L.tsem_destroy.restype = None
    L.tsem_last_error.argtypes = [vp]
    L.tsem_last_error.restype = C.c_char_p
    L.tsem_set_stream.argtypes = [vp, vp]
    L.tsem_set_option.argtypes = [vp, C.c_char_p, i64]
    L.tsem_synchronize.argtypes = [vp]
    L.tsem_load_scores.argtypes = [vp, i64, i32, vp, vp, vp, vp, i32]
    L.tsem_generate.argtypes = [vp, i64, i64, i32, vp, i32, u64, i32, dbl]
    L.tsem_max_score.argtypes = [vp, C.POINTER(i32)]
    L.tsem_set_lut.argtypes = [vp, vp, i32]
    L.tsem_score_lut.argtypes = [i32, C.c_double, vp]
    L.tsem_dims.argtypes = [vp, C.POINTER(i64), C.POINTER(i32), C.POINTER(i64)]
    L.tsem_export_csr.argtypes = [vp, vp, vp, vp]
    L.tsem_rowstats.argtypes = [vp, vp, vp, vp, vp]
    L.tsem_export_rowinfo.argtypes = [vp, vp, vp]
    L.tsem_set_model.argtypes = [vp, vp, vp, vp, vp, dbl, dbl]
    L.tsem_set_params.argtypes = [vp, vp, vp]
    L.tsem_get_params.argtypes = [vp, C.c_int, vp, vp]
    L.tsem_reduce_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(i64)]
    L.tsem_bind_reduce_buffer.argtypes = [vp, vp, i64]
    L.tsem_em_pass.argtypes = [vp]
    L.tsem_em_update.argtypes = [vp, C.POINTER(dbl)]
    L.tsem_lnl_pass.argtypes = [vp]
    L.tsem_read_reduce.argtypes = [vp, vp, i64, i64]
    L.tsem_em_steps.argtypes = [vp, i32, vp]
    L.tsem_em_chunk.argtypes = [vp, i32, dbl, i32, i32, C.POINTER(i32), C.POINTER(i32), vp, vp, C.POINTER(dbl)]
    L.tsem_prepare_likelihood.argtypes = [vp]
    L.tsem_fallback_twopass.argtypes = [vp]
    L.tsem_recover_timeout.argtypes = [vp, C.POINTER(i32)]
    L.tsem_final_lnl.argtypes = [vp, C.POINTER(dbl)]
    L.tsem_comm_unique_id.argtypes = [vp]
    L.tsem_comm_create.argtypes = [C.POINTER(vp), C.c_int, vp, C.c_int, C.c_int]
    L.tsem_comm_destroy.argtypes = [vp]
    L.tsem_comm_destroy.restype = None
    L.tsem_comm_last_error.argtypes = []
    L.tsem_comm_last_error.restype = C.c_char_p
    L.tsem_comm_attach.argtypes = [vp, vp]
    L.tsem_comm_allreduce.argtypes = [vp, i64, i64]
    L.tsem_comm_allreduce_host.argtypes = [vp, vp, i64, C.c_int]
    L.tsem_comm_library_info.argtypes = [C.c_char_p, i32]
    L.tsem_comm_local_group.argtypes = [C.POINTER(vp), C.c_int, C.c_int]
    L.tsem_comm_local_group_destroy.argtypes = [vp]
    L.tsem_comm_local_group_destroy.restype = None
    L.tsem_comm_create_local.argtypes = [C.POINTER(vp), vp, C.c_int]
    L.tsem_comm_local_group_set_timeout.argtypes = [vp, dbl]
    L.tsem_set_prev_lnl.argtypes = [vp, dbl]
    L.tsem_legacy_randint.argtypes = [vp, C.POINTER(i32), vp, i64, vp]
    L.tsem_em_run.argtypes = [vp, dbl, i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(dbl),
                              vp, vp, vp, vp]
    L.tsem_export_z.argtypes = [vp, C.c_int, vp]
    L.tsem_estep.argtypes = [vp, vp, vp, vp]
    L.tsem_set_user_z.argtypes = [vp, vp]
    L.tsem_mstep.argtypes = [vp, vp, vp, vp]
    L.tsem_calc_lnl.argtypes = [vp, vp, vp, vp, C.POINTER(dbl)]
    L.tsem_best_counts.argtypes = [vp, C.c_int, vp]
    L.tsem_best_ties.argtypes = [vp, C.c_int, i64, vp, vp, C.POINTER(i64)]
    L.tsem_report_colsums.argtypes = [vp, C.c_int, C.c_double, vp, C.POINTER(i64)]
    L.tsem_report_ties.argtypes = [vp, i64, vp, vp]
    L.tsem_reassign_rows.argtypes = [vp, C.c_int, C.c_double, C.c_int, vp, vp, i64, vp]
    L.tsem_reassign.argtypes = [vp, C.c_int, dbl, C.c_int, vp, vp, vp]
    L.tsem_rows_lookup.argtypes = [vp, C.c_int, C.c_int, dbl, i64, vp, vp, vp, vp, vp]
    L.tsem_entry_tags.argtypes = [vp, C.c_int, C.c_int, dbl, vp, i64, i64, vp, i32, vp]
    L.tsem_entry_tags_end.argtypes = [vp]
    L.tsem_reassign_groups.argtypes = [vp, C.c_int, dbl, C.c_int, vp, vp, C.c_int32, vp]
    L.tsem_set_groups.argtypes = [vp, vp, C.c_int32]
    L.tsem_group_counts.argtypes = [vp, C.c_int, dbl, C.c_int, vp, C.POINTER(i64)]
    L.tsem_group_counts_copy.argtypes = [vp, vp, vp, vp]
    L.tsem_group_counts_shape.argtypes = [vp, C.POINTER(i32), C.POINTER(i64)]
    L.tsem_cell_em.argtypes = [vp, dbl, i32, i32]
    L.tsem_cell_em_shape.argtypes = [vp, C.POINTER(i32), C.POINTER(i64)]
    L.tsem_cell_em_copy.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.tsem_bootstrap.argtypes = [vp, i32, u64, vp, i32, dbl, dbl, i32]
    L.tsem_bootstrap_copy.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.tsem_bootstrap_mult.argtypes = [vp, u64, i32, i64, i64, vp]
    L.tsem_bootstrap_groups.argtypes = [vp, i32, u64, vp, i32, dbl, dbl, i32, i32, C.POINTER(i64)]
    L.tsem_bootstrap_groups_shape.argtypes = [vp, C.POINTER(i32), C.POINTER(i64), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.tsem_bootstrap_groups_copy.argtypes = [vp, vp, vp, vp, vp, vp]
    L.tsem_umi_dedup.argtypes = [vp, vp, vp, i32, i32, vp, vp]
    L.tsem_bam_scan.argtypes = [vp, i64, vp, i64, C.POINTER(i64), C.POINTER(i64)]
    L.tsem_bam_open.argtypes = [C.POINTER(vp), C.c_int, i32, vp, vp, i64, vp, vp, vp, vp, vp]
    L.tsem_bam_close.argtypes = [vp]
    L.tsem_bam_chunk.argtypes = [vp, vp, i64, vp, i64, i32, i32, i32, i32, i32, dbl, i32, vp, vp]
    L.tsem_bam_times.argtypes = [vp, C.c_int, vp, C.POINTER(i64)]
    L.tsem_bam_names.argtypes = [vp, vp, vp, i32]
    L.tsem_bam_rewrite_size.argtypes = [vp, vp, vp, vp]
    L.tsem_bam_update_size.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp]
    L.tsem_bam_rewrite_slots.argtypes = [vp, vp, vp, i64]
    L.tsem_bam_rewrite_fetch.argtypes = [vp, vp, i64, vp, i64]
    L.tsem_bam_rewrite_times.argtypes = [vp, C.c_int, vp, C.POINTER(i64)]
    L.tsem_bam_collate.argtypes = [C.c_int, vp, i64, vp, i64, i32, vp, vp, C.POINTER(i64), vp, vp]
    L.tsem_bam_collate_host.argtypes = [vp, i64, vp, i64, i32, vp, vp, C.POINTER(i64), vp]
    L.tsem_bgzf_scan.argtypes = [vp, i64, vp, i64, C.POINTER(i64), C.POINTER(i64), C.POINTER(i32)]
    L.tsem_bgzf_open.argtypes = [C.POINTER(vp), C.c_int]
    L.tsem_bgzf_close.argtypes = [vp]
    L.tsem_bgzf_inflate.argtypes = [vp, vp, i64, vp, i64, vp, i64, vp, vp, C.POINTER(i64)]
    L.tsem_bgzf_times.argtypes = [vp, C.c_int, vp, C.POINTER(i64)]
    L.tsem_bgzf_deflate.argtypes = [vp, vp, i64, vp, i64, C.POINTER(i64), C.POINTER(i64)]
    L.tsem_bgzf_deflate_host.argtypes = [vp, i64, vp, i64, C.POINTER(i64), C.POINTER(i64)]
    L.tsem_bgzf_deflate_times.argtypes = [vp, C.c_int, vp, C.POINTER(i64)]
    L.tsem_csr_norm_rows.argtypes = [C.c_int, i64, vp, vp, vp]
    L.tsem_csr_binmax_rows.argtypes = [C.c_int, i64, i32, vp, vp, vp]
    L.tsem_csr_scale.argtypes = [C.c_int, C.c_int, i64, i32, vp, vp, vp]
    L.tsem_kernel_stats.argtypes = [vp, C.c_int, C.POINTER(dbl), C.POINTER(i64), C.POINTER(i64)]
    L.tsem_report_stats.argtypes = [vp, C.POINTER(dbl), C.POINTER(i64), C.POINTER(i64), C.POINTER(C.c_int32)]
    L.tsem_phase_times.argtypes = [vp, C.c_int, vp, C.POINTER(i64)]
    L.tsem_device_memory.argtypes = [vp, C.c_int, C.POINTER(i64), C.POINTER(i64), vp]
    L.tsem_layout_info.argtypes = [vp, vp]
    L.tsem_layout_info_n.argtypes = [vp, vp, i32]
    L.tsem_report_info_n.argtypes = [vp, vp, i32]
    L.tsem_debug_fused_prof.argtypes = [vp, vp]
    L.tsem_debug_fused_startup.argtypes = [vp, vp]
    L.tsem_debug_log1p.argtypes = [C.c_int, C.c_int32, vp, vp]
    L.tsem_debug_log1p_tab.argtypes = [C.c_int, C.c_int32, vp, vp]
    L.tsem_debug_log1p_of_log.argtypes = [C.c_int, C.c_int32, vp, vp, vp, vp, vp]
    L.tsem_debug_phred.argtypes = [C.c_int, C.c_int32, vp, vp, C.c_int32, vp]
    L.tsem_debug_stream_read.argtypes = [C.c_int, i64, i32, C.POINTER(dbl)]
    L.tsem_debug_subblock.argtypes = [vp, C.c_int64, C.c_int32, vp, C.c_int64]
    L.tsem_debug_idx24.argtypes = [vp, vp, vp]
    L.tsem_debug_quad64.argtypes = [vp, vp, vp, C.c_uint64, vp]
    L.tsem_debug_fused_cell.argtypes = [C.c_int32] * 6 + [vp, vp]
    L.tsem_debug_fused_lds.argtypes = [C.c_int32] * 12 + [vp] * 5
    L.tsem_debug_subblock_values.argtypes = [vp, C.c_int64, C.c_int32, vp, vp, vp, C.c_int64]
    L.tsem_debug_fused_launches.argtypes = [vp, vp, C.c_int64]
    L.tsem_debug_fused_launches_clear.argtypes = [vp]
    L.tsem_debug_fused_census_index.argtypes = [C.c_int32] * 6
    L.tsem_debug_valmap.argtypes = [C.c_int32, vp]
    L.tsem_quad_order_host.argtypes = [C.c_int64, vp, vp, vp]
    for name in exported_symbols():
        fn = getattr(L, name)
        if name not in ('tsem_destroy', 'tsem_last_error', 'tsem_comm_destroy', 'tsem_comm_last_error',
                        'tsem_debug_subblock', 'tsem_debug_subblock_values', 'tsem_comm_local_group_destroy'):
            fn.restype = C.c_int
    L.tsem_debug_subblock.restype = C.c_int64
    L.tsem_debug_subblock_values.restype = C.c_int64
    _lib = L
    return L


def ptr(a):
    """Raw pointer of a C-contiguous numpy array (None -> NULL)."""
    if a is None:
        return None
    assert a.flags['C_CONTIGUOUS']
    return a.ctypes.data_as(C.c_void_p)


class Engine(object):
    """One handle == one GPU.  Thin, typed wrapper over the C ABI."""

    def __init__(self, device=0):
        L = lib()
        h = C.c_void_p()
        rc = L.tsem_create(C.byref(h), int(device))
        if rc != OK:
            raise EngineError('tsem_create failed (%d): %s — the EM engine needs an MI355X HIP '
                              'device; there is no CPU fallback.'
                              % (rc, L.tsem_last_error(None).decode()))
        self._L, self._h, self.device = L, h, device

    def close(self):
        if getattr(self, '_h', None):
            self._L.tsem_destroy(self._h)
            self._h = None

    __del__ = close

    def _ck(self, rc):
        if rc != OK:
            e = EngineError('libtelescope_em error %d: %s' % (rc, self._L.tsem_last_error(self._h).decode()))
            e.code = rc
            raise e

    # -- plumbing --
    def set_stream(self, stream_handle):
        self._ck(self._L.tsem_set_stream(self._h, C.c_void_p(stream_handle)))

    def set_option(self, key, value):
        self._ck(self._L.tsem_set_option(self._h, key.encode(), int(value)))
        self.__dict__.setdefault('options', {})[key] = int(value)      # (what was set: em() restores "kernel_timing")

    def synchronize(self):
        self._ck(self._L.tsem_synchronize(self._h))

    # -- matrix --
    def load_scores(self, indptr, indices, raw, n_cols, lut):
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        raw = np.ascontiguousarray(raw, dtype=np.uint16)
        if lut is None:                                   # the table follows: max_score() -> set_lut()
            self._ck(self._L.tsem_load_scores(self._h, len(indptr) - 1, int(n_cols), ptr(indptr), ptr(indices),
                                              ptr(raw), None, 0))
            return
        lut = np.ascontiguousarray(lut, dtype=np.float64)
        self._ck(self._L.tsem_load_scores(self._h, len(indptr) - 1, int(n_cols), ptr(indptr), ptr(indices),
                                          ptr(raw), ptr(lut), len(lut)))

    def generate(self, row_begin, row_end, n_cols, len_cdf, seed, dist, uniq_frac):
        len_cdf = np.ascontiguousarray(len_cdf, dtype=np.uint32)
        self._ck(self._L.tsem_generate(self._h, int(row_begin), int(row_end), int(n_cols), ptr(len_cdf),
                                       len(len_cdf), int(seed), int(dist), float(uniq_frac)))

    def max_score(self):
        m = C.c_int32()
        self._ck(self._L.tsem_max_score(self._h, C.byref(m)))
        return m.value

    def set_lut(self, lut):
        lut = np.ascontiguousarray(lut, dtype=np.float64)
        self._ck(self._L.tsem_set_lut(self._h, ptr(lut), len(lut)))

    def dims(self):
        n, k, z = C.c_int64(), C.c_int32(), C.c_int64()
        self._ck(self._L.tsem_dims(self._h, C.byref(n), C.byref(k), C.byref(z)))
        return n.value, k.value, z.value

    def export_csr(self):
        n, k, nnz = self.dims()
        indptr = np.empty(n + 1, np.int64)
        indices = np.empty(nnz, np.int32)
        raw = np.empty(nnz, np.uint16)
        self._ck(self._L.tsem_export_csr(self._h, ptr(indptr), ptr(indices), ptr(raw)))
        return indptr, indices, raw

    # -- model --
    def rowstats(self):
        _, k, _ = self.dims()
        stats, pisum0 = np.zeros(3), np.zeros(k)
        cnt, hsh = np.zeros(k, np.uint64), np.zeros(k, np.uint64)
        self._ck(self._L.tsem_rowstats(self._h, ptr(stats), ptr(pisum0), ptr(cnt), ptr(hsh)))
        return stats, pisum0, cnt, hsh

    def row_info(self):
        """(Y uint8[N], weights f64[N]) of the local rows as the device holds them (model.py:679,690)."""
        n, _, _ = self.dims()
        y, w = np.zeros(n, np.uint8), np.zeros(n)
        self._ck(self._L.tsem_export_rowinfo(self._h, ptr(y), ptr(w)))
        return y, w

    def set_model(self, stats, pisum0, col_count, col_hash, pi_prior, theta_prior):
        stats = np.ascontiguousarray(stats, dtype=np.float64)
        pisum0 = np.ascontiguousarray(pisum0, dtype=np.float64)
        col_count = np.ascontiguousarray(col_count, dtype=np.uint64)
        col_hash = np.ascontiguousarray(col_hash, dtype=np.uint64)
        self._ck(self._L.tsem_set_model(self._h, ptr(stats), ptr(pisum0), ptr(col_count), ptr(col_hash),
                                        float(pi_prior), float(theta_prior)))

    def set_params(self, pi, theta):
        pi = np.ascontiguousarray(pi, dtype=np.float64)
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        self._ck(self._L.tsem_set_params(self._h, ptr(pi), ptr(theta)))

    def get_params(self, which=Z_CUR):
        _, k, _ = self.dims()
        pi, theta = np.empty(k), np.empty(k)
        self._ck(self._L.tsem_get_params(self._h, which, ptr(pi), ptr(theta)))
        return pi, theta

    # -- EM --
    def reduce_buffer(self):
        p, n = C.c_void_p(), C.c_int64()
        self._ck(self._L.tsem_reduce_buffer(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def bind_reduce_buffer(self, dptr, count):
        self._ck(self._L.tsem_bind_reduce_buffer(self._h, C.c_void_p(dptr), int(count)))

    def em_pass(self):
        self._ck(self._L.tsem_em_pass(self._h))

    def em_update(self, want_diff=True):
        d = C.c_double()
        self._ck(self._L.tsem_em_update(self._h, C.byref(d) if want_diff else None))
        return d.value

    def lnl_pass(self):
        self._ck(self._L.tsem_lnl_pass(self._h))

    def read_reduce(self, offset, count):
        out = np.empty(count)
        self._ck(self._L.tsem_read_reduce(self._h, ptr(out), int(offset), int(count)))
        return out

    def em_steps(self, n, want_diffs=True):
        out = np.empty(n) if want_diffs else None
        self._ck(self._L.tsem_em_steps(self._h, int(n), ptr(out)))
        return out

    def em_chunk(self, n_max, epsilon=0.0, use_likelihood=False, first=False, last=False):
        """Up to `n_max` iterations of the em() loop body enqueued back to back; convergence is decided on
        the device (include/telescope_em.h).  Returns (diffs, lnls, stopped) of the committed iterations.
        With `use_likelihood` on a layout prepared for it (`prepare_likelihood`) the lnl of the chunk's last
        iteration is NaN unless `last` (it comes with the next chunk: `self.lnl_carry`, NaN when nothing was owed)."""
        n_max = int(n_max)
        diffs, lnls = np.empty(max(1, n_max)), np.empty(max(1, n_max))
        done, stopped, carry = C.c_int32(), C.c_int32(), C.c_double(float('nan'))
        self._ck(self._L.tsem_em_chunk(self._h, n_max, float(epsilon), int(bool(use_likelihood)), int(bool(first)) | (2 if last else 0),
                                       C.byref(done), C.byref(stopped), ptr(diffs), ptr(lnls), C.byref(carry)))
        n = done.value
        self.lnl_carry = carry.value
        return diffs[:n], (lnls[:n] if use_likelihood else None), bool(stopped.value)

    def prepare_likelihood(self):
        """em(use_likelihood=True): lay the matrix out so that the EM pass carries the previous iteration's log-likelihood
        (a no-op when it is, or cannot be; include/telescope_em.h)."""
        self._ck(self._L.tsem_prepare_likelihood(self._h))

    def set_prev_lnl(self, lnl):
        """The lnl the next run's first iteration is compared with under use_likelihood (model.py:786)."""
        self._ck(self._L.tsem_set_prev_lnl(self._h, float(lnl)))

    def final_lnl(self):
        out = C.c_double()
        self._ck(self._L.tsem_final_lnl(self._h, C.byref(out)))
        return out.value

    def fallback_twopass(self):
        self._ck(self._L.tsem_fallback_twopass(self._h))

    def recover_timeout(self):
        sw = C.c_int32()
        self._ck(self._L.tsem_recover_timeout(self._h, C.byref(sw)))
        return bool(sw.value)

    def comm_attach(self, comm_handle):
        self._ck(self._L.tsem_comm_attach(self._h, comm_handle))

    def comm_allreduce(self, offset, count):
        self._ck(self._L.tsem_comm_allreduce(self._h, int(offset), int(count)))

    def em_run(self, epsilon, max_iter, use_likelihood):
        _, k, _ = self.dims()
        n_iter, conv, lnl = C.c_int32(), C.c_int32(), C.c_double()
        diffs, lnls = np.full(max_iter, np.nan), np.full(max_iter, np.nan)
        pi0, th0 = np.empty(k), np.empty(k)
        self._ck(self._L.tsem_em_run(self._h, float(epsilon), int(max_iter), int(bool(use_likelihood)),
                                     C.byref(n_iter), C.byref(conv), C.byref(lnl), ptr(diffs), ptr(lnls),
                                     ptr(pi0), ptr(th0)))
        n = n_iter.value
        return dict(n_iter=n, converged=bool(conv.value), lnl=lnl.value, diffs=diffs[:n],
                    lnls=lnls[:n], pi_init=pi0, theta_init=th0)

    # -- results --
    def export_z(self, which=Z_PREV):
        _, _, nnz = self.dims()
        z = np.empty(nnz)
        self._ck(self._L.tsem_export_z(self._h, which, ptr(z)))
        return z

    def set_user_z(self, z_aligned):
        if z_aligned is not None:
            z_aligned = np.ascontiguousarray(z_aligned, dtype=np.float64)
        self._ck(self._L.tsem_set_user_z(self._h, ptr(z_aligned)))

    def estep(self, pi, theta):
        _, _, nnz = self.dims()
        pi = np.ascontiguousarray(pi, dtype=np.float64)
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        z = np.empty(nnz)
        self._ck(self._L.tsem_estep(self._h, ptr(pi), ptr(theta), ptr(z)))
        return z

    def mstep(self, z_aligned):
        _, k, _ = self.dims()
        z_aligned = np.ascontiguousarray(z_aligned, dtype=np.float64)
        pi, theta = np.empty(k), np.empty(k)
        self._ck(self._L.tsem_mstep(self._h, ptr(z_aligned), ptr(pi), ptr(theta)))
        return pi, theta

    def calc_lnl(self, z_aligned, pi, theta):
        z_aligned = np.ascontiguousarray(z_aligned, dtype=np.float64)
        pi = np.ascontiguousarray(pi, dtype=np.float64)
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        out = C.c_double()
        self._ck(self._L.tsem_calc_lnl(self._h, ptr(z_aligned), ptr(pi), ptr(theta), C.byref(out)))
        return out.value

    def best_counts(self, which):
        n, _, _ = self.dims()
        nb = np.empty(n, np.int32)
        self._ck(self._L.tsem_best_counts(self._h, which, ptr(nb)))
        return nb

    def best_ties(self, which):
        """(rows, counts) of the rows with several best hits, in row order (compacted on the device)."""
        n = C.c_int64()
        cap = 1 << 16
        while True:
            rows, counts = np.empty(cap, np.int32), np.empty(cap, np.int32)
            rc = self._L.tsem_best_ties(self._h, which, cap, ptr(rows), ptr(counts), C.byref(n))
            if rc == OK:
                return rows[:n.value].copy(), counts[:n.value].copy()
            if rc == ERR_ARG and n.value > cap:
                cap = int(n.value)
                continue
            self._ck(rc)

    def report_colsums(self, which, thresh):
        """One pass: {'conf', 'exclude', 'average'} column sums of z(`which`) and the tied rows (rows, counts) in row order."""
        _, k, _ = self.dims()
        out = np.empty(3 * k)
        n = C.c_int64()
        self._ck(self._L.tsem_report_colsums(self._h, which, float(thresh), ptr(out), C.byref(n)))
        rows, counts = np.empty(n.value, np.int32), np.empty(n.value, np.int32)
        self._ck(self._L.tsem_report_ties(self._h, n.value, ptr(rows), ptr(counts)))
        return {'conf': out[:k], 'exclude': out[k:2 * k], 'average': out[2 * k:]}, rows, counts

    def reassign_rows(self, method, thresh, which, rows, picks, n=None):
        """Column sums of reassign(method) restricted to a list of rows (rows=None: the tie rows of the last report)."""
        _, k, _ = self.dims()
        cs = np.empty(k)
        if rows is not None:
            rows = np.ascontiguousarray(rows, dtype=np.int32); n = len(rows)
        pk = np.ascontiguousarray(picks, dtype=np.int32) if picks is not None else None
        self._ck(self._L.tsem_reassign_rows(self._h, RA_CODE[method], float(thresh), which,
                                            ptr(rows) if rows is not None else None,
                                            ptr(pk) if pk is not None else None, int(n), ptr(cs)))
        return cs

    def reassign(self, method, thresh, which, picks=None, want_mask=False):
        n, k, nnz = self.dims()
        cs = np.empty(k)
        mask = np.empty(nnz) if want_mask else None
        if picks is not None:
            picks = np.ascontiguousarray(picks, dtype=np.int32)
        self._ck(self._L.tsem_reassign(self._h, RA_CODE[method], float(thresh), which, ptr(picks), ptr(cs),
                                       ptr(mask)))
        return cs, mask

    def rows_lookup(self, method, thresh, which, rows, out_off, picks=None, want_z=True, want_mask=True):
        """(z, mask) of the entries of the listed rows, compact (tsem_rows_lookup): row rows[i] -> [out_off[i], out_off[i + 1])."""
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        out_off = np.ascontiguousarray(out_off, dtype=np.int64)
        total = int(out_off[-1]) if len(out_off) else 0
        z = np.zeros(total) if want_z else None
        m = np.zeros(total) if want_mask else None
        pk = None if picks is None else np.ascontiguousarray(picks, dtype=np.int32)
        self._ck(self._L.tsem_rows_lookup(self._h, which, RA_CODE[method], float(thresh), len(rows), ptr(rows), ptr(pk), ptr(out_off),
                                          ptr(z), ptr(m)))
        return z, m

    def entry_tags(self, method, thresh, which, row_begin, row_end, phred_tab, picks=None, n_out=None):
        """uint32 tag word of every stored entry of rows [row_begin, row_end) (tsem_entry_tags); `n_out` = their count."""
        tab = np.ascontiguousarray(phred_tab, dtype=np.float64)
        pk = None if picks is None else np.ascontiguousarray(picks, dtype=np.int32)
        out = np.empty(int(n_out), dtype=np.uint32)
        self._ck(self._L.tsem_entry_tags(self._h, which, RA_CODE[method], float(thresh), ptr(pk), int(row_begin), int(row_end),
                                         ptr(tab), len(tab), ptr(out)))
        return out

    def entry_tags_end(self):
        self._ck(self._L.tsem_entry_tags_end(self._h))

    def set_groups(self, group_of_row, n_groups):
        """Row -> group map of the per-group sums, copied to the device once (None drops it)."""
        self.groups_token = None          # whoever sets a map may tag it afterwards (TelescopeLikelihood: a digest of the grouping)
        if group_of_row is None:
            self._ck(self._L.tsem_set_groups(self._h, None, 0))
            return
        n, _, _ = self.dims()
        grp = np.ascontiguousarray(group_of_row, dtype=np.int32)
        if grp.shape != (n,):
            raise ValueError('group_of_row must have one entry per row')
        self._ck(self._L.tsem_set_groups(self._h, ptr(grp), int(n_groups)))

    def reassign_groups(self, method, thresh, which, group_of_row, n_groups, picks=None, out=None):
        """[n_groups][K] sums of the assignment over the rows of each group; `group_of_row` None = the map of `set_groups`."""
        n, k, _ = self.dims()
        grp = None
        if group_of_row is not None:
            self.groups_token = None      # the call replaces the resident map
            grp = np.ascontiguousarray(group_of_row, dtype=np.int32)
            if grp.shape != (n,):
                raise ValueError('group_of_row must have one entry per row')
        if out is None:
            out = np.zeros((int(n_groups), k))
        if picks is not None:
            picks = np.ascontiguousarray(picks, dtype=np.int32)
        self._ck(self._L.tsem_reassign_groups(self._h, RA_CODE[method], float(thresh), which, ptr(picks), ptr(grp),
                                              int(n_groups), ptr(out)))
        return out

    def group_counts(self, method, thresh, which, picks=None):
        """Sparse per-group sums of the assignment over the map of `set_groups` (tsem_group_counts): (group_ptr int64 [n_groups + 1],
        cols int32 [nnz], vals float64 [nnz]) — a CSR matrix with columns ascending within a group."""
        n, _, _ = self.dims()
        if picks is not None:
            picks = np.ascontiguousarray(picks, dtype=np.int32)
            if picks.shape != (n,):
                raise ValueError('picks must have one entry per row')
        nnz, n_groups = C.c_int64(), C.c_int32()
        self._ck(self._L.tsem_group_counts(self._h, RA_CODE[method], float(thresh), which, ptr(picks), C.byref(nnz)))
        self._ck(self._L.tsem_group_counts_shape(self._h, C.byref(n_groups), C.byref(nnz)))   # (the arrays are sized by the library)
        gptr = np.empty(n_groups.value + 1, np.int64)
        cols, vals = np.empty(nnz.value, np.int32), np.empty(nnz.value)
        self._ck(self._L.tsem_group_counts_copy(self._h, ptr(gptr), ptr(cols), ptr(vals)))
        return gptr, cols, vals

    def cell_em(self, epsilon, max_iter, use_likelihood=False):
        """One EM fit per group of the map of `set_groups` (tsem_cell_em); the per-cell final z becomes the Z_USER buffer.  Returns
        the arrays of tsem_cell_em_copy as a dict."""
        self._ck(self._L.tsem_cell_em(self._h, float(epsilon), int(max_iter), int(bool(use_likelihood))))
        n_cells, n_cols = C.c_int32(), C.c_int64()
        self._ck(self._L.tsem_cell_em_shape(self._h, C.byref(n_cells), C.byref(n_cols)))
        g, nc = n_cells.value, n_cols.value
        r = dict(col_ptr=np.empty(g + 1, np.int64), cols=np.empty(nc, np.int32), pi=np.empty(nc), theta=np.empty(nc),
                 pi_init=np.empty(nc), theta_init=np.empty(nc), rest=np.empty((g, 4)), n_iter=np.empty(g, np.int32),
                 converged=np.empty(g, np.int32), lnl=np.empty(g))
        self._ck(self._L.tsem_cell_em_copy(self._h, *[ptr(r[k]) for k in ('col_ptr', 'cols', 'pi', 'theta', 'pi_init', 'theta_init',
                                                                         'rest', 'n_iter', 'converged', 'lnl')]))
        return r

    def bootstrap(self, n_rep, seed, mult, method, thresh, epsilon, max_iter, n_cols):
        """`n_rep` bootstrap refits (tsem_bootstrap); `mult` None (the device draws Poisson(1) multiplicities from `seed`) or a
        uint8 [n_rep x N] array.  Returns the arrays of tsem_bootstrap_copy as a dict, `info` = (batch, hot columns)."""
        if mult is not None:
            mult = np.ascontiguousarray(mult, dtype=np.uint8)
        self._ck(self._L.tsem_bootstrap(self._h, int(n_rep), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(mult), RA_CODE[method], float(thresh),
                                        float(epsilon), int(max_iter)))
        b, k = int(n_rep), int(n_cols)
        r = dict(pi=np.empty((b, k)), theta=np.empty((b, k)), counts=np.empty((b, k)), n_frags=np.empty(b, np.int64),
                 n_iter=np.empty(b, np.int32), converged=np.empty(b, np.int32), lnl=np.empty(b), info=np.zeros(2, np.int32))
        self._ck(self._L.tsem_bootstrap_copy(self._h, *[ptr(r[key]) for key in ('pi', 'theta', 'counts', 'n_frags', 'n_iter', 'converged',
                                                                               'lnl', 'info')]))
        return r

    def bootstrap_groups(self, n_rep, seed, mult, method, thresh, epsilon, max_iter, n_cols, keep_values=False):
        """The replicates of `bootstrap` — the same dict — fitted once, with per-group statistics over the map of `set_groups`
        (tsem_bootstrap_groups) under key `groups`: a dict of group_ptr int64 [n_groups + 1], cols int32 [nnz], mean, sd float64 [nnz],
        n_used, and values float64 [n_rep x nnz] or None."""
        if mult is not None:
            mult = np.ascontiguousarray(mult, dtype=np.uint8)
        nnz = C.c_int64()
        self._ck(self._L.tsem_bootstrap_groups(self._h, int(n_rep), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(mult), RA_CODE[method],
                                               float(thresh), float(epsilon), int(max_iter), int(bool(keep_values)), C.byref(nnz)))
        b, k = int(n_rep), int(n_cols)
        r = dict(pi=np.empty((b, k)), theta=np.empty((b, k)), counts=np.empty((b, k)), n_frags=np.empty(b, np.int64),
                 n_iter=np.empty(b, np.int32), converged=np.empty(b, np.int32), lnl=np.empty(b), info=np.zeros(2, np.int32))
        self._ck(self._L.tsem_bootstrap_copy(self._h, *[ptr(r[key]) for key in ('pi', 'theta', 'counts', 'n_frags', 'n_iter', 'converged',
                                                                               'lnl', 'info')]))
        n_groups, n_reps, n_used, kept = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self._ck(self._L.tsem_bootstrap_groups_shape(self._h, C.byref(n_groups), C.byref(nnz), C.byref(n_reps), C.byref(n_used),
                                                     C.byref(kept)))             # (the arrays are sized by the library)
        s = nnz.value
        g = dict(group_ptr=np.empty(n_groups.value + 1, np.int64), cols=np.empty(s, np.int32), mean=np.empty(s), sd=np.empty(s),
                 n_used=int(n_used.value), values=np.empty((n_reps.value, s)) if kept.value else None)
        self._ck(self._L.tsem_bootstrap_groups_copy(self._h, ptr(g['group_ptr']), ptr(g['cols']), ptr(g['mean']), ptr(g['sd']),
                                                    ptr(g['values'])))
        r['groups'] = g
        return r

    def bootstrap_mult(self, seed, rep, row_begin, row_end):
        """The multiplicities the device draws for replicate `rep`, rows [row_begin, row_end) (tsem_bootstrap_mult)."""
        out = np.empty(max(0, int(row_end) - int(row_begin)), np.uint8)
        self._ck(self._L.tsem_bootstrap_mult(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(rep), int(row_begin), int(row_end), ptr(out)))
        return out

    def umi_dedup(self, cell_of_row, umi_of_row, n_cells, n_umis):
        """The representative of every row's UMI component (tsem_umi_dedup): (rep int32 [N], stats int64 [4] = rows in classes,
        classes, components among them, rows dropped).  Row i is kept iff rep[i] == i."""
        n, _, _ = self.dims()
        cor = np.ascontiguousarray(cell_of_row, dtype=np.int32)
        uor = np.ascontiguousarray(umi_of_row, dtype=np.int32)
        if cor.shape != (n,) or uor.shape != (n,):
            raise ValueError('cell_of_row and umi_of_row must have one entry per row')
        rep, stats = np.empty(n, np.int32), np.zeros(4, np.int64)
        self._ck(self._L.tsem_umi_dedup(self._h, ptr(cor), ptr(uor), int(n_cells), int(n_umis), ptr(rep), ptr(stats)))
        return rep, stats

    # -- instrumentation --
    def kernel_stats(self, reset=False):
        ms, n, b = C.c_double(), C.c_int64(), C.c_int64()
        self._ck(self._L.tsem_kernel_stats(self._h, int(reset), C.byref(ms), C.byref(n), C.byref(b)))
        return dict(em_ms=ms.value, em_launches=n.value, algo_bytes_per_pass=b.value)

    def report_stats(self):
        """The last report_colsums: dict(kernel_ms (option kernel_timing != 0), algo_bytes, deferred_rows, kernel)."""
        ms, b, d, k = C.c_double(), C.c_int64(), C.c_int64(), C.c_int32()
        self._ck(self._L.tsem_report_stats(self._h, C.byref(ms), C.byref(b), C.byref(d), C.byref(k)))
        return dict(kernel_ms=ms.value, algo_bytes=b.value, deferred_rows=d.value,
                    kernel={0: None, 1: 'k_rowpass', 2: 'k_report_rows', 3: 'k_report_init_codes', 4: 'k_report_pack32'}[k.value])

    def report_info(self):
        """Which kernel instance served the last report_colsums ('colsums') and the last reassign_groups ('groups', its last tile):
        tsem_report_info_n.  Per call a dict of kernel (as report_stats names it; 'k_group_unique' too), G, E, initial, group_mode,
        cold, Hs, HC, lut_rep, grid, block, deferred_long, deferred_near (-1: no list), tiles, tile_groups."""
        info = np.zeros(32, np.int64)
        self._ck(self._L.tsem_report_info_n(self._h, ptr(info), info.size))
        names = ('kernel', 'G', 'E', 'initial', 'group_mode', 'cold', 'Hs', 'HC', 'lut_rep', 'grid', 'block', 'deferred_long',
                 'deferred_near', 'tiles', 'tile_groups')
        kern = {0: None, 1: 'k_rowpass', 2: 'k_report_rows', 3: 'k_report_init_codes', 4: 'k_report_pack32', 5: 'k_group_unique'}
        out = {}
        for key, half in (('colsums', info[:16]), ('groups', info[16:])):
            d = dict(zip(names, half.tolist()))
            d['kernel'] = kern[d['kernel']]
            out[key] = d
        return out

    def device_memory(self):
        """dict(free, total, resident=dict(csr, csr_indices, ids, layout, rows)) in bytes."""
        f, t = C.c_int64(), C.c_int64()
        r = np.zeros(5, np.int64)
        self._ck(self._L.tsem_device_memory(self._h, 0, C.byref(f), C.byref(t), ptr(r)))
        return dict(free=f.value, total=t.value, resident=dict(zip(('csr', 'csr_indices', 'ids', 'layout', 'rows'), r.tolist())))

    def phase_times(self, reset=False):
        """Option 'phase_timing': mean microseconds per chunked iteration of pass / column reduce / all-reduce / update, the gap
        to the next iteration, and first-to-last mark; None when nothing was timed."""
        ms, n = np.zeros(6), C.c_int64()
        self._ck(self._L.tsem_phase_times(self._h, int(reset), ptr(ms), C.byref(n)))
        if n.value == 0:
            return None
        us = ms * 1e3 / n.value
        return dict(iterations=int(n.value), **{k: float(v) for k, v in zip(('pass', 'colreduce', 'allreduce', 'update', 'gaps', 'iteration'), us)})

    def fused_prof(self):
        out = np.zeros((64, 16), np.uint64)
        self._ck(self._L.tsem_debug_fused_prof(self._h, ptr(out)))
        return out

    def fused_startup(self):
        """Start-up timeline of the last profiled fused launch: [workgroup][entry, counted, zeroed, tables, loop start, loop end, exit, id]
        in 10 ns ticks (include/telescope_em.h)."""
        out = np.zeros((512, 8), np.uint64)
        self._ck(self._L.tsem_debug_fused_startup(self._h, ptr(out)))
        return out

    def debug_subblock(self, block, part, cap=8192):
        out = np.zeros(cap, np.uint32)
        n = self._L.tsem_debug_subblock(self._h, int(block), int(part), ptr(out), cap)
        if n < 0:
            raise EngineError('tsem_debug_subblock failed (%d)' % n)
        return out[:n]

    def debug_subblock_values(self, block, part, cap=8192):
        """(values, rows, cols) of a sub-block in entry order: entry e is word e of `debug_subblock`; rows / cols are the CSR row
        and the column its word names.  Padding has value 0."""
        out, rows, cols = np.zeros(cap, np.float64), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        n = self._L.tsem_debug_subblock_values(self._h, int(block), int(part), ptr(out), ptr(rows), ptr(cols), cap)
        if n < 0:
            raise EngineError('tsem_debug_subblock_values failed (%d)' % n)
        return out[:n], rows[:n], cols[:n]

    def fused_launches(self):
        """The launch census of this handle (tsem_debug_fused_launches; host only): {cell: (n, n_conditional)} over the cells of the
        fused kernel's table that were launched since the counters were cleared — cell = (team size, mode, entry format, geometry,
        timeline, index format); n the launches that ran unconditionally, n_conditional those enqueued with the device's choice
        between the two forms of the lnl pass armed."""
        out = np.zeros(2 * len(FUSED_CELLS), np.int64)
        self._ck(self._L.tsem_debug_fused_launches(self._h, ptr(out), out.size))
        return {FUSED_CELLS[c]: (int(out[2 * c]), int(out[2 * c + 1])) for c in np.flatnonzero(out.reshape(-1, 2).any(axis=1)).tolist()}

    def clear_fused_launches(self):
        self._ck(self._L.tsem_debug_fused_launches_clear(self._h))

    def layout_info(self, extended=False):
        """Facts about the resident layout (include/telescope_em.h, tsem_layout_info_n).  extended: also the values appended behind
        the first 40 — the index format in use, its dummy entries, the pack kernel's count of unrepresentable quads and the auto
        rule's size threshold, the conflict-aware entry order applied (0 none, 1 the score-code walk, 2 the quad order) and the
        quads the quad order permuted."""
        info = np.zeros(46 if extended else 40, np.int64)
        self._ck(self._L.tsem_layout_info_n(self._h, ptr(info), info.size))
        return dict(zip(('P', 'Kp', 'R', 'nb', 'N_amb', 'N_uni', 'nnz_amb', 'nnz_pad', 'twin_cols',
                         'G1', 'G2', 'fused', 'slow_path', 'max_subblock', 'value_bytes', 'hot_cols',
                         'lds_bytes', 'row_order', 'geometry', 'fallbacks', 'bin_repeats', 'reproducible', 'exact_single', 'lnl_fused', 'split', 'single_part_rows', 'row_pass_em', 'lnl_tables', 'lnl_linear', 'lnl_mid_entries', 'lnl_mid_limit', 'near_tie_rows', 'index_bytes',
                         'cell_em_wave', 'cell_em_256', 'cell_em_512', 'cell_em_global', 'cell_em_spread',
                         'rowstats_lanes', 'colsig_lanes',
                         'index_format', 'index_dummies', 'index_unrepresentable', 'index_auto_min_bytes',
                         'order_kind', 'order_quads_moved'), info.tolist()))


def quad_order_host(words):
    """The conflict-aware order inside quads (csrc/tsem_quadorder.h) on the host: `words` holds whole windows of 64 local row << 16 |
    local column words.  Returns (codes, moved): one permutation code per quad — entry (code >> 2 j) & 3 goes to position j — and the
    number of quads that change."""
    words = np.ascontiguousarray(words, np.uint32).ravel()
    if words.size % 64:
        raise ValueError('whole windows of 64 entries')
    codes = np.zeros(max(1, words.size // 4), np.uint8)
    moved = C.c_int64(0)
    rc = lib().tsem_quad_order_host(words.size // 64, ptr(words) if words.size else ptr(np.zeros(1, np.uint32)), ptr(codes), C.byref(moved))
    if rc != OK:
        raise EngineError('tsem_quad_order_host failed (%d)' % rc)
    return codes[:words.size // 4], int(moved.value)


def legacy_randint(counts):
    """`np.random.randint(0, counts)` on numpy's GLOBAL legacy RandomState — the same picks, the same state afterwards
    — by the library's C loop (tsem_legacy_randint): three times faster than numpy's per-element path, which matters
    for the millions of tied rows `choose` draws for."""
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    out = np.empty(counts.size, np.int32)
    if counts.size == 0:
        return out
    st = np.random.get_state()
    if st[0] != 'MT19937':
        raise RuntimeError('numpy legacy RandomState is not MT19937')
    key = np.array(st[1], dtype=np.uint32, copy=True)
    pos = C.c_int32(int(st[2]))
    rc = lib().tsem_legacy_randint(ptr(key), C.byref(pos), ptr(counts), counts.size, ptr(out))
    if rc != OK:
        raise ValueError('low >= high')                     # what numpy raises for a count < 1
    # (the cached Gaussian belongs to other distributions' draws: untouched by integer draws, kept as it is)
    np.random.set_state((st[0], key, pos.value) + tuple(st[3:]))
    return out


def comm_library_info():
    """Which RCCL the library resolved at run time: 'rccl <version> (<path>)', or why none is available."""
    buf = C.create_string_buffer(1024)
    lib().tsem_comm_library_info(buf, 1024)
    return buf.value.decode()


class LocalGroup(object):
    """In-process transport (include/telescope_em.h): `world` engines on ONE device, one host thread each."""

    def __init__(self, device, world):
        L = lib()
        g = C.c_void_p()
        rc = L.tsem_comm_local_group(C.byref(g), int(device), int(world))
        if rc != OK:
            raise EngineError('tsem_comm_local_group failed (%d): %s' % (rc, L.tsem_comm_last_error().decode()))
        self._L, self.handle, self.device, self.world = L, g, device, world

    def comm(self, rank):
        return LibComm(self.device, None, rank, self.world, group=self)

    def set_timeout(self, seconds):
        """How long a rank waits for its peers at a collective before it fails (default 120 s)."""
        rc = self._L.tsem_comm_local_group_set_timeout(self.handle, float(seconds))
        if rc != OK:
            raise EngineError('tsem_comm_local_group_set_timeout failed (%d)' % rc)

    def close(self):
        if getattr(self, 'handle', None):
            self._L.tsem_comm_local_group_destroy(self.handle)
            self.handle = None


class LibComm(object):
    """The library's own communicator.  RCCL (one per process / GPU): `unique_id()` on rank 0, ship the 128
    bytes to the other ranks, then `LibComm(device, id, rank, world)` everywhere (collective).  In-process
    transport: `LocalGroup(device, world).comm(rank)`."""
    ID_BYTES = 128
    _DT = {('f64', 'sum'): 0, ('u64', 'sum'): 1, ('f64', 'max'): 2, ('i64', 'max'): 3}

    @staticmethod
    def unique_id():
        buf = np.zeros(LibComm.ID_BYTES, np.uint8)
        rc = lib().tsem_comm_unique_id(ptr(buf))
        if rc != OK:
            raise EngineError('tsem_comm_unique_id failed (%d): %s' % (rc, lib().tsem_comm_last_error().decode()))
        return buf.tobytes()

    def __init__(self, device, unique_id, rank, world, group=None):
        L = lib()
        h = C.c_void_p()
        if group is not None:
            rc = L.tsem_comm_create_local(C.byref(h), group.handle, int(rank))
            self._group = group                               # keeps the group alive
        else:
            idb = np.frombuffer(unique_id, np.uint8).copy()
            rc = L.tsem_comm_create(C.byref(h), int(device), ptr(idb), int(rank), int(world))
        if rc != OK:
            raise EngineError('tsem_comm_create failed (%d): %s' % (rc, L.tsem_comm_last_error().decode()))
        self._L, self.handle, self.rank, self.world, self.device = L, h, rank, world, device

    def allreduce(self, a, kind='f64', op='sum'):
        dt = {'f64': np.float64, 'u64': np.uint64, 'i64': np.int64}[kind]
        a = np.array(a, dtype=dt, copy=True).ravel()
        rc = self._L.tsem_comm_allreduce_host(self.handle, ptr(a), a.size, self._DT[(kind, op)])
        if rc != OK:
            raise EngineError('tsem_comm_allreduce_host failed (%d): %s' % (rc, self._L.tsem_comm_last_error().decode()))
        return a

    def close(self):
        if getattr(self, 'handle', None):
            self._L.tsem_comm_destroy(self.handle)
            self.handle = None

    __del__ = close


def debug_log1p(x, device=0, table=False):
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.empty_like(x)
    rc = (lib().tsem_debug_log1p_tab if table else lib().tsem_debug_log1p)(device, len(x), ptr(x), ptr(y))
    if rc != OK:
        raise EngineError('tsem_debug_log1p failed (%d)' % rc)
    return y


def debug_phred(p, phred_tab, device=0):
    """The tag pass's PHRED lookup (tsem_debug_phred) of every p."""
    p = np.ascontiguousarray(p, dtype=np.float64)
    tab = np.ascontiguousarray(phred_tab, dtype=np.float64)
    out = np.empty(len(p), dtype=np.int32)
    rc = lib().tsem_debug_phred(device, len(p), ptr(p), ptr(tab), len(tab), ptr(out))
    if rc != OK:
        raise EngineError('tsem_debug_phred failed (%d)' % rc)
    return out


def debug_log1p_of_log(q, c, device=0):
    """log1p(q * c) as the log-table lnl passes form it from log q and log c (tsem_fused.h, fz_log1p_of_log)."""
    q = np.ascontiguousarray(q, dtype=np.float64)
    c = np.ascontiguousarray(c, dtype=np.float64)
    with np.errstate(divide='ignore'):
        lq, lc = np.log(q), np.log(c)
    y = np.zeros_like(q)
    rc = lib().tsem_debug_log1p_of_log(device, len(q), ptr(lq), ptr(lc), ptr(q), ptr(c), ptr(y))
    if rc != OK:
        raise EngineError('tsem_debug_log1p_of_log failed (%d)' % rc)
    return y


def device_memory(device=0):
    """(free, total) bytes of a device's memory, without an engine."""
    f, t = C.c_int64(), C.c_int64()
    if lib().tsem_device_memory(None, int(device), C.byref(f), C.byref(t), None) != OK:
        raise EngineError('tsem_device_memory failed (no usable HIP device?)')
    return f.value, t.value


def stream_read_gbs(device=0, nbytes=8 << 30, reps=3):
    """GB/s a pure streaming read reaches on this GPU (tsem_debug_stream_read)."""
    g = C.c_double()
    rc = lib().tsem_debug_stream_read(device, int(nbytes), int(reps), C.byref(g))
    if rc:
        raise EngineError('tsem_debug_stream_read failed (%d)' % rc)
    return g.value


BAM_COLS = 34                  # TSEM_BAM_COLS; the rows of BamLoader.chunk's matrix (include/telescope_em.h)
BAM_STATUS = {1: 'block_size does not match the record chain', 2: 'l_read_name leaves the record', 3: 'n_cigar runs past the record',
              4: 'l_seq runs past the record', 5: 'an aux field begins past the record', 6: 'an aux value runs past the record',
              7: 'a Z / H aux value has no NUL inside the record', 8: 'a B aux array runs past the record',
              9: 'unknown aux type', 10: 'a mapped alignment has no AS tag'}


# status words of tsem_bgzf_inflate (include/telescope_em.h, telescope_amd/csrc/tsem_bgzf_inflate.h); 255: left to the host
BGZF_HOST = 255
BGZF_STATUS = {1: 'DEFLATE block type 3', 2: 'a stored block whose LEN does not match NLEN',
               3: 'an over-subscribed or incomplete Huffman code', 4: 'no code for end-of-block', 5: 'an invalid literal/length or distance symbol',
               6: 'a distance before the start of the output', 7: 'the output is longer than ISIZE', 8: 'the compressed bytes end inside the stream',
               9: 'the output is shorter than ISIZE', 10: 'CRC-32 mismatch'}


def bgzf_scan(data, cap=None):
    """Block table of a piece of a BGZF file (tsem_bgzf_scan, host only): (int64 [n][5] = block offset, payload offset, payload length,
    ISIZE, CRC-32; consumed; not_bgzf)."""
    buf = np.frombuffer(data, dtype=np.uint8)
    cap = buf.size // 26 + 1 if cap is None else int(cap)
    blk = np.empty((cap, 5), np.int64)
    n, used, nb = C.c_int64(), C.c_int64(), C.c_int32()
    rc = lib().tsem_bgzf_scan(ptr(buf) if buf.size else None, buf.size, ptr(blk), cap, C.byref(n), C.byref(used), C.byref(nb))
    if rc != OK:
        raise _csr_error('tsem_bgzf_scan', rc)
    return blk[:n.value].copy(), used.value, bool(nb.value)


class _StageHandle(object):
    """A handle of the device loader's units (tsem_bgzf_*, tsem_bam_*): opened through a tsem_*_open, closed through the class's
    `_close` when the object is closed or collected; its stage times read through a tsem_*_times."""

    _close = None

    def _open(self, fn, *args):
        L = lib()
        h = C.c_void_p()
        rc = getattr(L, fn)(C.byref(h), *args)
        if rc != OK:
            raise _csr_error(fn, rc)
        self._L, self._h = L, h

    def close(self):
        if getattr(self, '_h', None):
            getattr(self._L, self._close)(self._h)
            self._h = None

    __del__ = close

    def _times(self, fn, names, count_key, reset):
        """{name: HIP-event milliseconds summed over the calls so far, count_key: their number}"""
        ms, n = np.zeros(len(names)), C.c_int64()
        rc = getattr(self._L, fn)(self._h, int(reset), ptr(ms), C.byref(n))
        if rc != OK:
            raise _csr_error(fn, rc)
        return dict(zip(names, ms.tolist()), **{count_key: n.value})


class BgzfInflater(_StageHandle):
    """The device side of `--inflate device` (tsem_bgzf_open / tsem_bgzf_inflate): one handle, one GPU, its buffers kept between batches."""

    _close = 'tsem_bgzf_close'

    def __init__(self, device=0):
        self._open('tsem_bgzf_open', int(device))

    def inflate(self, data, blocks):
        """-> (uint8 array of the inflated bytes of the blocks that are not left to the host, in order; int32 status per block;
        (code, block) of the first failing block or (0, -1))."""
        buf = np.frombuffer(data, dtype=np.uint8)
        blk = np.ascontiguousarray(blocks, dtype=np.int64).reshape(-1, 5)
        n = len(blk)
        isz = blk[:, 3]
        cap = int(isz[isz <= 65536].sum())
        out = np.empty(cap, np.uint8)
        st = np.zeros(n, np.int32)
        first, total = np.zeros(2, np.int64), C.c_int64()
        rc = self._L.tsem_bgzf_inflate(self._h, ptr(buf) if buf.size else None, buf.size, ptr(blk) if n else None, n, ptr(out) if cap else None,
                                       cap, ptr(st) if n else None, ptr(first), C.byref(total))
        if rc != OK:
            raise _csr_error('tsem_bgzf_inflate', rc)
        assert total.value == cap
        return out, st, (int(first[0]), int(first[1]))

    def times(self, reset=False):
        """HIP-event milliseconds summed over the batches so far, and their number."""
        return self._times('tsem_bgzf_times', ('h2d', 'k_bgzf_inflate', 'd2h'), 'batches', reset)


BGZF_BLOCK_IN = 0xff00                  # input bytes per block of the deflate entries (bam_out._BLOCK_IN)


def _bgzf_deflate_call(fn, name, handle, stream):
    buf = np.frombuffer(stream, dtype=np.uint8)
    nb = (buf.size + BGZF_BLOCK_IN - 1) // BGZF_BLOCK_IN
    cap = buf.size + 31 * nb
    out = np.empty(cap, np.uint8)
    n_out, n_blk = C.c_int64(), C.c_int64()
    args = (ptr(buf) if buf.size else None, buf.size, ptr(out) if cap else None, cap, C.byref(n_out), C.byref(n_blk))
    rc = fn(*(((handle,) if handle is not None else ()) + args))
    if rc != OK:
        raise _csr_error(name, rc)
    assert n_blk.value == nb and n_out.value <= cap
    return out[:n_out.value]


def bgzf_deflate_host(stream):
    """The BGZF blocks (no EOF block) of a byte stream cut every 0xff00 bytes, by the kernel's body with one lane on the CPU
    (tsem_bgzf_deflate_host, no device): uint8 array, the bytes that BgzfDeflater.deflate gives."""
    return _bgzf_deflate_call(lib().tsem_bgzf_deflate_host, 'tsem_bgzf_deflate_host', None, stream)


class BgzfDeflater(_StageHandle):
    """The device side of `--deflate device` (tsem_bgzf_open / tsem_bgzf_deflate): one handle, one GPU, its buffers kept between batches."""

    _close = 'tsem_bgzf_close'

    def __init__(self, device=0):
        self._open('tsem_bgzf_open', int(device))

    def deflate(self, stream):
        """-> uint8 array: the BGZF blocks of `stream` (cut every 0xff00 bytes, the last one shorter), one behind the other; no EOF block"""
        return _bgzf_deflate_call(self._L.tsem_bgzf_deflate, 'tsem_bgzf_deflate', self._h, stream)

    def times(self, reset=False):
        """HIP-event milliseconds summed over the batches so far, and their number."""
        return self._times('tsem_bgzf_deflate_times', ('h2d', 'k_bgzf_deflate', 'pack', 'd2h'), 'batches', reset)


def bam_scan(data, cap=None):
    """Record offsets of a chunk of inflated BAM bytes (tsem_bam_scan, host only): (rec_off int64 [n + 1], consumed)."""
    buf = np.frombuffer(data, dtype=np.uint8)
    cap = buf.size // 36 + 1 if cap is None else int(cap)
    off = np.empty(cap + 1, np.int64)
    n, used = C.c_int64(), C.c_int64()
    rc = lib().tsem_bam_scan(ptr(buf) if buf.size else None, buf.size, ptr(off), cap, C.byref(n), C.byref(used))
    if rc != OK:
        raise _csr_error('tsem_bam_scan', rc)
    return off[:n.value + 1].copy(), used.value


COLLATE_STATUS = {1: 'the record is shorter than its fixed fields and one byte of a name', 2: 'l_read_name is 0',
                  3: 'the name runs past the end of the record'}


def bam_collate(data, rec_off, device=None, hash_bits=0):
    """The records of an inflated BAM record stream brought together by name (tsem_bam_collate on GPU `device`; device=None:
    tsem_bam_collate_host, the same bodies on one CPU thread): the groups of equal names in the order of their first records, the
    records of a group in their input order.  `rec_off` as bam_scan gives it.  -> (uint8 array of the collated stream, order int64 [n]
    = the input index of every output record, the number of names, ms) with ms = the HIP-event milliseconds of h2d / hash_insert_key /
    sort_scan / gather / d2h, None on the host.  A record that cannot be collated is a ValueError that names it.  `hash_bits` (tests):
    keep so many bits of the names' hash, 0 = all.  The device holds the stream twice and 44 to 60 B per record during the call."""
    buf = np.frombuffer(data, dtype=np.uint8)
    off = np.ascontiguousarray(rec_off, dtype=np.int64)
    n = len(off) - 1
    if n < 0:
        raise ValueError('rec_off holds n + 1 offsets')
    out, order = np.empty(buf.size, np.uint8), np.empty(n, np.int64)
    names, st = C.c_int64(), np.zeros(2, np.int64)
    args = (ptr(buf) if buf.size else None, buf.size, ptr(off), n, int(hash_bits), ptr(out) if buf.size else None, ptr(order) if n else None,
            C.byref(names), ptr(st))
    if device is None:
        ms = None
        rc = lib().tsem_bam_collate_host(*args)
    else:
        ms = np.zeros(5)
        rc = lib().tsem_bam_collate(int(device), *(args + (ptr(ms),)))
    if rc == ERR_NOMEM:
        e = EngineError('--collate device: the inflated BAM (%d bytes, %d records) does not fit: the step holds the whole stream twice and '
                        '44 to 60 B per record in device memory (%s); collate the file beforehand, or use --collate host'
                        % (buf.size, n, lib().tsem_last_error(None).decode()))
        e.code = rc
        raise e
    if rc != OK:
        raise _csr_error('tsem_bam_collate' if device is not None else 'tsem_bam_collate_host', rc)
    if st[0]:
        raise ValueError('record %d: %s' % (int(st[1]), COLLATE_STATUS.get(int(st[0]), 'status %d' % int(st[0]))))
    total = int(off[n] - off[0])
    if ms is not None:
        ms = dict(zip(('h2d', 'hash_insert_key', 'sort_scan', 'gather', 'd2h'), ms.tolist()))
    return out[:total], order, names.value, ms


def _tag16(tag):
    if tag is None:
        return -1
    t = tag.encode()
    if len(t) != 2:
        raise ValueError('a BAM tag has two letters, not %r' % tag)
    return t[0] | (t[1] << 8)


class BamLoader(_StageHandle):
    """The device side of the device loader (tsem_bam_open / tsem_bam_chunk): the annotation's arrays on one GPU and the four
    kernels per chunk.  `ref_lo`, `ref_hi` per BAM reference; `starts`, `maxend`, `ends`, `locus`, `strand` per interval."""

    _close = 'tsem_bam_close'

    def __init__(self, device, ref_lo, ref_hi, starts, maxend, ends, locus, strand):
        a = [np.ascontiguousarray(x, dtype=t) for x, t in ((ref_lo, np.int32), (ref_hi, np.int32), (starts, np.int64), (maxend, np.int64),
                                                           (ends, np.int64), (locus, np.int32), (strand, np.int8))]
        self._open('tsem_bam_open', int(device), len(a[0]), ptr(a[0]), ptr(a[1]), len(a[2]), *[ptr(x) for x in a[2:]])

    def chunk(self, data, rec_off, barcode_tag=None, umi_tag=None, run_stranded=False, stranded_mode='None', overlap_threshold=0.2,
              record_cap=4096):
        """-> (int32 [BAM_COLS][n_rec], (status code, record)) of one chunk: the raw outputs of the four kernels."""
        buf = np.frombuffer(data, dtype=np.uint8)
        off = np.ascontiguousarray(rec_off, dtype=np.int64)
        n = len(off) - 1
        out = np.empty((BAM_COLS, max(n, 0)), np.int32)
        st = np.zeros(2, np.int64)
        rc = self._L.tsem_bam_chunk(self._h, ptr(buf) if buf.size else None, buf.size, ptr(off), n, _tag16(barcode_tag), _tag16(umi_tag),
                                    int(bool(run_stranded)), int(stranded_mode[0] == 'F'), int(stranded_mode[-1] == 'F'),
                                    float(overlap_threshold), int(record_cap), ptr(out), ptr(st))
        if rc != OK:
            raise _csr_error('tsem_bam_chunk', rc)
        return out, (int(st[0]), int(st[1]))

    def times(self, reset=False):
        """HIP-event milliseconds summed over the chunks so far, and their number."""
        return self._times('tsem_bam_times', ('h2d', 'k_bam_decode', 'k_bam_pair', 'k_bam_overlap', 'k_bam_fragment', 'd2h'), 'chunks', reset)

    # ---- the BAMs of --updated_sam (tsem_bam_names / _rewrite_size / _update_size / _rewrite_slots / _rewrite_fetch)
    def names(self, names):
        """The locus names in the order of their ids, the no_feature_key last (what the load stage writes as ZF / ZB)."""
        enc = [n.encode() for n in names]
        off = np.zeros(len(enc) + 1, np.int64)
        np.cumsum([len(e) for e in enc], out=off[1:])
        buf = np.frombuffer(b''.join(enc), dtype=np.uint8)
        rc = self._L.tsem_bam_names(self._h, ptr(buf) if buf.size else None, ptr(off), len(enc))
        if rc != OK:
            raise _csr_error('tsem_bam_names', rc)

    def rewrite_size(self, n):
        """Load stage, over the chunk of the last `chunk` call (n records) -> (pos_other, pos_tmp int64 [n + 1], (status code, record))"""
        po, pt, st = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64), np.zeros(2, np.int64)
        rc = self._L.tsem_bam_rewrite_size(self._h, ptr(po), ptr(pt), ptr(st))
        if rc != OK:
            raise _csr_error('tsem_bam_rewrite_size', rc)
        return po, pt, (int(st[0]), int(st[1]))

    def update_size(self, data, rec_off, words):
        """Update stage: a chunk of tmp records and their words -> (pos int64 [n + 1], (status code, record))"""
        buf = np.frombuffer(data, dtype=np.uint8)
        off = np.ascontiguousarray(rec_off, dtype=np.int64)
        w = np.ascontiguousarray(words, dtype=np.uint32)
        n = len(off) - 1
        if len(w) != n:
            raise ValueError('one word per record: %d words, %d records' % (len(w), n))
        pos, st = np.zeros(n + 1, np.int64), np.zeros(2, np.int64)
        rc = self._L.tsem_bam_update_size(self._h, ptr(buf) if buf.size else None, buf.size, ptr(off), n, ptr(w) if n else None, ptr(pos), ptr(st))
        if rc != OK:
            raise _csr_error('tsem_bam_update_size', rc)
        return pos, (int(st[0]), int(st[1]))

    def rewrite_slots(self, n):
        """(kind, pair slot) int32 [n] of the last sizing call, before its fetch"""
        kind, pair = np.empty(n, np.int32), np.empty(n, np.int32)
        rc = self._L.tsem_bam_rewrite_slots(self._h, ptr(kind), ptr(pair), n)
        if rc != OK:
            raise _csr_error('tsem_bam_rewrite_slots', rc)
        return kind, pair

    def rewrite_fetch(self, n_other, n_tmp):
        """The streams of the last sizing call: (other, tmp) uint8 arrays of exactly these lengths"""
        other, tmp = np.empty(int(n_other), np.uint8), np.empty(int(n_tmp), np.uint8)
        if n_other or n_tmp:
            rc = self._L.tsem_bam_rewrite_fetch(self._h, ptr(other) if n_other else None, int(n_other), ptr(tmp) if n_tmp else None, int(n_tmp))
            if rc != OK:
                raise _csr_error('tsem_bam_rewrite_fetch', rc)
        return other, tmp

    def rewrite_times(self, reset=False):
        return self._times('tsem_bam_rewrite_times', ('h2d', 'k_bam_rw_plan', 'k_bam_rw_size', 'k_bam_rw_write', 'd2h'), 'calls', reset)


def _csr_error(fn, rc):
    e = EngineError('%s failed (%d): %s' % (fn, rc, lib().tsem_last_error(None).decode()))
    e.code = rc
    return e


def csr_norm_rows(indptr, data, device=0):
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    data = np.ascontiguousarray(data, dtype=np.float64)
    out = np.empty_like(data)
    rc = lib().tsem_csr_norm_rows(device, len(indptr) - 1, ptr(indptr), ptr(data), ptr(out))
    if rc != OK:
        raise _csr_error('tsem_csr_norm_rows', rc)
    return out


def csr_binmax_rows(indptr, data, n_cols, device=0):
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    data = np.ascontiguousarray(data, dtype=np.float64)
    out = np.empty(len(data), np.int8)
    rc = lib().tsem_csr_binmax_rows(device, len(indptr) - 1, int(n_cols), ptr(indptr), ptr(data), ptr(out))
    if rc != OK:
        raise _csr_error('tsem_csr_binmax_rows', rc)
    return out


def csr_scale(mode, indptr, data, n_cols, device=0):
    """mode 0: norm(); 1: scale(); 2: scale(1)  (sparse_plus.py:46-52, 93-97)."""
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    data = np.ascontiguousarray(data, dtype=np.float64)
    out = np.empty_like(data)
    rc = lib().tsem_csr_scale(device, int(mode), len(indptr) - 1, int(n_cols), ptr(indptr), ptr(data), ptr(out))
    if rc != OK:
        raise _csr_error('tsem_csr_scale', rc)
    return out
