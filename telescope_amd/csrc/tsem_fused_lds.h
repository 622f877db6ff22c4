// The dynamic LDS of k_em_fused (tsem_fused.h): ONE description of its regions.  The kernel takes every region pointer from it, the
// host takes the bytes to launch with, the row slots that fit and the room the log-Q table may take from it (tsem_internal.h).
//
//   region   doubles                      who uses it
//   c        kt                           pi*theta of the part (not MODE 7)
//   acc      kt                           the accumulators; lnl passes: pi*theta (or its logarithm) of the current parameters.  MODE 5
//                                         and 7 keep ONE table: acc is c
//   acc2     Kp                           MODE 3: the low pieces' accumulators; MODE 4: pi*theta of the previous parameters
//   y        yr * R                       partial row sums, a ring yr blocks deep (fz_yr)
//   s        2 * R                        w_i / rowsum_i, a ring of two blocks
//   rp       (sr - 2) * R                 MODE 4: 1 / rowsum_i of the previous pass, a ring of two blocks
//   ibox     FZ_LDS_IBOX                  16 ints: the ticket, the eight XCD counts
//   offs     FZ_LDS_OFFS                  [8][2] uint32: sub-block quad ranges
//   dum      FZ_LDS_DUM                   one double per lane: where idle lanes send their (zero) atomics
//   lut      lut_len                      FMT 1, 2: the score table
//   lq       lq_n                         MODE 9: log Q behind the score table (not when log Q is arithmetic: FMT 1 with lq_lin)
//   tail     exps: uint16 [Kp]            MODE 2, 3: the slots' exponent bounds
//            logtab: double2 [FZ_LOGTAB]  MODE 1, 9, 4, 8: (1 / c_i, log c_i) of fz_log1p_tab, on a 16-byte boundary
// The two tails share one place: no launch has both.
#pragma once

constexpr int FZ_LOGTAB = 64;
constexpr int FZ_LDS_IBOX = 16 * 4 / 8, FZ_LDS_OFFS = 8 * 2 * 4 / 8, FZ_LDS_DUM = 64;   // the fixed regions, in doubles
constexpr int FZ_LDS_TAIL_ALIGN = 16;   // bytes kept ahead of the tail for its round-up to a 16-byte boundary
constexpr int FZ_LDS_SPARE = 64;        // bytes no region takes: the launch size has carried them since the fixed regions were first
                                        // counted (192 B for the 128 of ibox and offs), and every layout's R and lds_bytes hang on it
constexpr int FZ_TAIL_NONE = 0, FZ_TAIL_EXPS = 1, FZ_TAIL_LOG = 2;

struct FzLdsIn {
  int ntab;      // tables of kt entries ahead of the rings
  int kt;        // entries per table: Kp; Kp + 2 bounds what the split layout's passes take; Kh in MODE 8
  int Kp;        // columns of the part (acc2, the exponent table)
  int yr, sr;    // depth of the y ring (fz_yr) and of the s / rp rings together (2, or 4 with rp)
  int R;
  int lut_len;   // entries of the score table in LDS
  int lq_n;      // entries of the log-Q table in LDS
  int tail;      // FZ_TAIL_*
};
// Where each region starts.  T = int: in doubles from the start of the dynamic LDS (the host).  T = double*: the pointers themselves,
// from the kernel's base — the same sums, so the kernel's address arithmetic is the chain of pointer sums it has always been.
template <typename T> struct FzLdsMap {
  T c, acc, acc2, y, s, rp, ibox, offs, dum, lut, lq, exps, logtab;
  int end;                 // BYTES to launch with: the tail's end, FZ_LDS_TAIL_ALIGN allowed for its round-up, and FZ_LDS_SPARE
};
__host__ __device__ constexpr int fz_lds_align16(int d) { return (d + 1) & ~1; }   // (the base is 16-byte aligned)
__host__ __device__ inline double* fz_lds_align16(double* p) { return reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(p) + 15) & ~(uintptr_t)15); }
template <typename T> __host__ __device__ constexpr FzLdsMap<T> fz_lds_map(T base, const FzLdsIn& in) {
  FzLdsMap<T> m = {};
  m.c = base;
  m.acc = in.ntab == 1 ? m.c : m.c + in.kt;
  m.acc2 = m.acc + in.Kp;
  m.y = m.acc + (in.ntab == 3 ? 2 : 1) * in.kt;
  m.s = m.y + in.yr * in.R;
  m.rp = m.s + 2 * in.R;
  m.ibox = m.s + in.sr * in.R;
  m.offs = m.ibox + FZ_LDS_IBOX;
  m.dum = m.offs + FZ_LDS_OFFS;
  m.lut = m.dum + FZ_LDS_DUM;
  m.lq = m.lut + in.lut_len;
  m.exps = m.lq + in.lq_n;
  m.logtab = fz_lds_align16(m.exps);
  m.end = (int)(m.exps - base) * 8 + FZ_LDS_SPARE + (in.tail == FZ_TAIL_NONE ? 0 : FZ_LDS_TAIL_ALIGN + (in.tail == FZ_TAIL_EXPS ? in.Kp * 2 : FZ_LOGTAB * 16));
  return m;
}
// Adaptor 1, per kernel: what the instantiation (MODE, FMT, GEO) launched with these arguments keeps in LDS (lut_len: FusedArgs'
// — 0 with FMT 0).  yr is fz_yr(GEO): the caller passes it, this header knows no geometry.
__host__ __device__ constexpr FzLdsIn fz_lds_kernel(int mode, int fmt, int yr, int Kp, int Kh, int R, int lut_len, int lq_n, int lq_lin) {
  FzLdsIn in = {};
  in.ntab = (mode == 5 || mode == 7) ? 1 : ((mode == 3 || mode == 4) ? 3 : 2);
  in.kt = mode == 8 ? Kh : Kp;
  in.Kp = Kp;
  in.yr = yr; in.sr = mode == 4 ? 4 : 2;
  in.R = R;
  in.lut_len = lut_len;
  in.lq_n = (mode == 9 && !(fmt == 1 && lq_lin)) ? lq_n : 0;
  in.tail = (mode == 2 || mode == 3) ? FZ_TAIL_EXPS : ((mode == 1 || mode == 9 || mode == 4 || mode == 8) ? FZ_TAIL_LOG : FZ_TAIL_NONE);
  return in;
}
// Adaptor 2, per layout: the bytes that hold every pass the layout can launch — what each of its fused launches asks for.  Plain
// values: the layout build drops `lnl3` and `exact_single` again when their kernels do not exist for the format it chose.
//   split: one table of Kp entries, or — its lnl pass — two of (Kp + 1) / 2;  exact_single / lnl3: a third table;  lnl3: the rp ring;
//   every layout runs an lnl pass (the log table), a reproducible one the exponent table too;  lut_len, lq_n: entries in LDS
__host__ __device__ constexpr int fz_lds_layout_bytes(int Kp, int R, int yr, bool split, bool exact_single, bool lnl3, bool reproducible,
                                                      int lut_len, int lq_n) {
  FzLdsIn in = {};
  in.ntab = split ? 1 : ((exact_single || lnl3) ? 3 : 2);
  in.kt = split ? Kp + 2 : Kp;
  in.Kp = Kp;
  in.yr = yr; in.sr = lnl3 ? 4 : 2;
  in.R = R;
  in.lut_len = lut_len; in.lq_n = lq_n;
  in.tail = FZ_TAIL_LOG;
  const int log_end = fz_lds_map(0, in).end;
  in.tail = FZ_TAIL_EXPS;
  const int exps_end = reproducible ? fz_lds_map(0, in).end : 0;
  return log_end > exps_end ? log_end : exps_end;
}
