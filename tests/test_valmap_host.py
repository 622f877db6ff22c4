"""The value map of the layouts the fused kernel reads (telescope_amd/csrc/tsem_valmap.h) on the host, no GPU: a numpy model of the map
as DESIGN.md 3 states it, for every sub-block size a register tile takes (16, 32, ... 896 quads), against

  * itself: a bijection onto the sub-block's bytes [0, 32 nq), every value on its own 8 bytes;
  * the fused kernel's addressing (tsem_fused.h, load_blk): wave w = tid >> 6 reads 16 bytes per lane at w * 2048 + lane * 16 and at
    w * 2048 + gq * 16 + lane * 16, each inside a resource that ends gq * 16 bytes behind the load's first byte of lane 0 — the two
    pieces of thread tid hold entries 4 tid .. 4 tid + 3 of the linear order, in that order; lanes past the sub-block's end are out of
    range in both; each load of a wave covers whole 128-byte lines;
  * the library: tsem_debug_valmap returns the positions the fill kernels and the read-back compute (the shared inline function)."""
import numpy as np
import pytest

NQS = list(range(16, 896 + 1, 16))
WAVES = 16                                        # a workgroup of 1024 threads: more threads than any register tile has quads


def model_bytes(nq):
    """byte offset of every entry e = 0 .. 4 nq - 1 from the sub-block's base"""
    e = np.arange(4 * nq, dtype=np.int64)
    q, k = e >> 2, e & 3
    g = q >> 6
    gq = np.minimum(64, nq - 64 * g)
    return g * 2048 + (k >> 1) * gq * 16 + (q & 63) * 16 + (k & 1) * 8


@pytest.mark.parametrize('nq', NQS)
def test_map_is_a_bijection_onto_the_sub_blocks_bytes(nq):
    b = model_bytes(nq)
    assert np.all(b % 8 == 0)
    assert np.array_equal(np.sort(b), np.arange(4 * nq, dtype=np.int64) * 8), 'every 8 bytes of [0, 32 nq) hold exactly one value'


@pytest.mark.parametrize('nq', NQS)
def test_every_lane_reads_its_four_consecutive_entries(nq):
    b = model_bytes(nq)
    entry_at = np.full(4 * nq, -1, dtype=np.int64)              # 8-byte slot -> entry
    entry_at[b // 8] = np.arange(4 * nq)
    for w in range(WAVES):
        gq = min(max(nq - 64 * w, 0), 64)                        # what the kernel forms in scalar registers
        base, bound = w * 2048, gq * 16                          # both resources: rebased to the group, gq * 16 bytes long
        for piece, shift in ((0, 0), (1, gq * 16)):
            lanes = np.arange(64)
            off = lanes * 16
            inside = off + 16 <= bound                            # the descriptor's bound: past it the hardware returns zeros
            tid = 64 * w + lanes
            assert np.array_equal(inside, tid < nq), (nq, w, piece)
            addr = base + shift + off[inside]
            assert np.all(addr + 16 <= 32 * nq), 'a load inside its resource stays inside the sub-block'
            got = np.stack([entry_at[addr // 8], entry_at[addr // 8 + 1]], axis=1)
            want = np.stack([4 * tid[inside] + 2 * piece, 4 * tid[inside] + 2 * piece + 1], axis=1)
            assert np.array_equal(got, want), (nq, w, piece)
            if gq:                                                # one contiguous run of whole 128-byte lines per instruction
                assert (base + shift) % 128 == 0 and (gq * 16) % 128 == 0
                assert np.array_equal(addr, base + shift + 16 * np.arange(gq))


def test_library_computes_the_model():
    from telescope_amd import _lib
    L = _lib.lib()
    for nq in NQS + [0]:
        pos = np.zeros(max(1, 4 * nq), np.uint32)
        assert L.tsem_debug_valmap(nq, _lib.ptr(pos)) == _lib.OK
        assert np.array_equal(pos[:4 * nq].astype(np.int64) * 8, model_bytes(nq)), nq
    for bad in (-16, 8, 17):
        assert L.tsem_debug_valmap(bad, _lib.ptr(np.zeros(128, np.uint32))) == _lib.ERR_ARG
