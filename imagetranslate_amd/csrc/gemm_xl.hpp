// The 256 x 256-tile main loop, written once for gemm_xl_kernel (gemm.hip), the fused scoring kernel (score.hip) and the k-NN
// kernel (knn.hip): tile geometry, the paired LDS-DMA issue, the per-wave 128 x 64 tile product, the wave roles, the K loop
// itself (xl_k_loop) and who owns which accumulator element (XlOwn); behind them the host-side checks that the launches of
// those kernels share.  knn_xl_kernel still carries its own copy of the loop and of the indices (it measured slower through
// these functions, see there).  See gemm.hip for the design notes.
#pragma once
#include "mma.hpp"

namespace {

constexpr int TILE_BYTES = 16384;            // one operand tile

template <typename T, bool KCONTIG> struct TileGeom {
  static constexpr int EPC = 16 / sizeof(T);                  // elements per 16-B chunk
  static constexpr int BK = 128 / sizeof(T);                  // K elements per tile
  static constexpr int RB = KCONTIG ? 128 : 128 * sizeof(T);  // LDS row bytes
  static constexpr int CPR = RB / 16;                         // chunks per row
};

constexpr int XL_THREADS = 512;
constexpr int XL_STAGE = 4 * TILE_BYTES;
constexpr int XL_LDS = 2 * XL_STAGE;

// One wave's share of TWO neighbouring 16-KiB sub-tiles (operand rows / columns +128): the second sub-tile's source
// offsets are the first's plus a constant, so a wave keeps 4 offset registers whichever operand it streams.
template <typename T> struct DmaPair {
  __amdgpu_buffer_rsrc_t rsrc;
  int voff[4], kadv, delta, wv;
  template <bool KCONTIG> IMT_DEVICE void init(const T* base, int64_t ld, int64_t valid_bytes, int row0, int wave) {
    typedef TileGeom<T, KCONTIG> G;
    rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(base), 0, (int)valid_bytes, 0x00020000);
    const int lane = threadIdx.x & 63;
    wv = wave;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = 64 * (4 * i + wave) + lane;
      const int tr = q / G::CPR, pc = q % G::CPR;
      const int c = pc ^ swz<G::RB>(tr);
      if (KCONTIG) voff[i] = (int)((((int64_t)(row0 + tr)) * ld + c * G::EPC) * (int64_t)sizeof(T));
      else         voff[i] = (int)((((int64_t)tr) * ld + row0 + c * G::EPC) * (int64_t)sizeof(T));
    }
    kadv = KCONTIG ? 128 : (int)(G::BK * ld * (int64_t)sizeof(T));
    delta = KCONTIG ? (int)(128 * ld * (int64_t)sizeof(T)) : (int)(128 * sizeof(T));
  }
  // The K advance and the +128-row delta are wave-uniform, but they go into the VECTOR offset: the descriptor's range
  // check (num_records = valid_bytes, which is what turns the rows past M of a ragged last tile into zeros instead of reads
  // past the operand) covers vgpr offset + instruction offset only -- the SGPR `soffset` operand is added AFTER the check
  // (tools/probe_soffset.hip; the round-1 fault of tools/probe_fill.hip was exactly an soffset beyond num_records).
  IMT_DEVICE void issue(char* tiles, int t) const {
    const int wave = __builtin_amdgcn_readfirstlane(wv);
    const int adv = __builtin_amdgcn_readfirstlane(t * kadv), d = __builtin_amdgcn_readfirstlane(delta);
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)(tiles + h * TILE_BYTES + (4 * i + wave) * 1024),
                                                 16, voff[i] + (adv + h * d), 0, 0, 0);
  }
};

template <typename T, int LAYOUT, int HALF = -1>
IMT_DEVICE void compute_tile_xl(f32x4 (&acc)[8][4], const char* ta, const char* tb, int wn) {
  constexpr bool A_KC = (LAYOUT != IMT_TN), B_KC = (LAYOUT == IMT_NT);
  typedef TileGeom<T, A_KC> GA;
  typedef TileGeom<T, B_KC> GB;
  typedef typename Frag<T>::type frag_t;
  constexpr int KSTEP = Frag<T>::KSTEP;
  constexpr int NSTEP = GA::BK / KSTEP;  // HALF = 0 / 1: the first / second half of the tile's K steps only
  constexpr int S0 = HALF == 1 ? NSTEP / 2 : 0, S1 = HALF == 0 ? NSTEP / 2 : NSTEP;
#pragma unroll
  for (int s = S0; s < S1; ++s) {
    frag_t fa[8], fb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (B_KC) fb[j] = lds_frag_kcontig<T, GB::RB>(tb, wn + 16 * j, 4 * s);
      else      fb[j] = KStrided<T, GB::RB>::load(tb, s * KSTEP, wn + 16 * j);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (A_KC) fa[i] = lds_frag_kcontig<T, GA::RB>(ta, 16 * i, 4 * s);
      else      fa[i] = KStrided<T, GA::RB>::load(ta, s * KSTEP, 16 * i);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) mma16(acc[i][j], fb[j], fa[i]);
    // keep the next K step's 12 fragment reads below this step's MFMAs: hoisted, they push the 128 accumulator
    // registers + 2 x 48 fragment registers past the 256 a wave gets at two waves per SIMD (spills in the loop)
    __builtin_amdgcn_sched_barrier(0);
  }
}

// The 8 waves of a workgroup as 2 (m) x 4 (n): wave (wmi, wni) multiplies rows 128 wmi .. +127 by columns 64 wni .. +63 of the
// tile (wn: that strip's offset inside its 128-column B sub-tile).  Waves 0-3 stream the A sub-tiles, waves 4-7 the B sub-tiles.
// Five wave-uniform scalars, which the epilogues take BY VALUE: handed a reference, the compiler laid out the last row group of
// score_tile_reduce differently and fused other multiply-adds of its log-sum-exp merge (1 ulp in a row's lse).
struct XlWave {
  int wave, wmi, wni, wn;
  bool loads_a;
  IMT_DEVICE XlWave() : wave(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)), wmi(wave >> 2), wni(wave & 3), wn((wni & 1) * 64), loads_a(wave < 4) {}
};

// Who owns what of acc[8][4], relative to the tile's origin: lane (lr, lg) of wave (wmi, wni) holds in acc[i][j][e] the
// product of row row(i) = 128 wmi + 16 i + lr and column col(j) + e = 64 wni + 16 j + 4 lg + e (C^T fragments: 4 consecutive
// columns of one row per lane; the 4 lanes lg of a row are 16 lanes apart, two xor-shuffles (16, 32) combine a row).
struct XlOwn {
  int lg, r0, c0;
  IMT_DEVICE explicit XlOwn(const XlWave w) : lg((threadIdx.x & 63) >> 4), r0(128 * w.wmi + (threadIdx.x & 15)), c0(64 * w.wni + 4 * lg) {}
  IMT_DEVICE int row(int i) const { return r0 + 16 * i; }
  IMT_DEVICE int col(int j) const { return c0 + 16 * j; }
};

IMT_DEVICE void xl_zero(f32x4 (&acc)[8][4]) {
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// acc += the product of K tiles kt0 .. kt0 + nt - 1 of the two operands behind `dma` (each wave's own DmaPair), in that order:
// its callers run THIS loop, so a product is the same bits whichever of them, and whichever split, computes it.
// dbg (tuning only, tools/xl_ablate.py; a literal 0 folds the branches away): bit0 skip the tile products, bit1 skip the
// in-loop DMA, bit6 all waves issue before their MFMAs.  on_tile(stage) runs after each tile's products, while the stage is
// still valid.
template <typename T, int LAYOUT, typename OnTile>
IMT_DEVICE void xl_k_loop(f32x4 (&acc)[8][4], char* smem, const DmaPair<T>& dma, const XlWave& w, int kt0, int nt, int dbg,
                          unsigned long long* trace, OnTile on_tile) {
  auto issue = [&](int slot, int t) { dma.issue(smem + slot * XL_STAGE + (w.loads_a ? 0 : 2 * TILE_BYTES), kt0 + t); };
  if (nt > 0) issue(0, 0);
  for (int t = 0; t < nt; ++t) {
    // my eight pieces of tile t have landed; the barrier publishes everyone's and proves that the other stage (read
    // while multiplying tile t-1) is free for the DMA of tile t+1
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_barrier" ::: "memory");
    // Issuing a wave's eight 1-KiB DMA pieces takes it ~0.4 us during which it multiplies nothing (one wave sustains
    // ~20 GB/s of LDS-DMA, profiles/r01_lds_fill_probe.txt).  Waves w and w+4 share a SIMD: the first issues before its
    // MFMAs, the second between its two K steps, so each SIMD always has one wave multiplying.
    const bool issue_now = (t + 1 < nt) && !(dbg & 2);
    if (issue_now && (w.wave < 4 || (dbg & 64))) issue((t + 1) & 1, t + 1);
    if (t == 0) IMT_STAMP(trace, 1);
    const char* st = smem + (t & 1) * XL_STAGE;
    if (!(dbg & 1)) compute_tile_xl<T, LAYOUT, 0>(acc, st + w.wmi * TILE_BYTES, st + (2 + (w.wni >> 1)) * TILE_BYTES, w.wn);
    if (issue_now && w.wave >= 4 && !(dbg & 64)) issue((t + 1) & 1, t + 1);
    if (!(dbg & 1)) compute_tile_xl<T, LAYOUT, 1>(acc, st + w.wmi * TILE_BYTES, st + (2 + (w.wni >> 1)) * TILE_BYTES, w.wn);
    on_tile(st);
  }
}

// ------------------------------------------------------------------------------------------------ host side of the launches
// bytes from the first to the last element of a [rows][inner] view with leading dimension ld: the range of its buffer descriptor
inline int64_t view_bytes(int rows, int64_t ld, int inner, int es) { return rows > 0 ? ((int64_t)(rows - 1) * ld + inner) * es : 0; }

// opt in to that much dynamic LDS, once per kernel: `static const bool ok = allow_lds(...)`; false = the device refused
template <typename K> bool allow_lds(K kernel, int bytes) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess;
}
#define IMT_CHECK_LDS(ok, who, bytes)                                                        \
  do {                                                                                        \
    if (!(ok)) {                                                                              \
      imt_set_error("%s: the device does not give a workgroup %d bytes of LDS", who, bytes);  \
      return IMT_ERR_LAUNCH;                                                                  \
    }                                                                                         \
  } while (0)

// One K-contiguous [rows][K] operand of the NT loop (x / w of imt_score_rows, x / y of imt_knn_rows) as its DMA wants it:
// rows that start on 16 bytes, and 32-bit byte offsets that still hold one ragged 256-row tile past the last row.
// who: the entry point, p_name / ld_name: the arguments, for the message.
inline int xl_check_rows(const char* who, const char* p_name, const char* ld_name, const void* p, int64_t ld, int rows, int K, int es) {
  IMT_CHECK_ARG(ld >= K && ld % (16 / es) == 0 && (uintptr_t)p % 16 == 0, "%s: %s / %s must keep rows 16-byte aligned", who, ld_name, p_name);
  IMT_CHECK_ARG(((int64_t)rows + 256) * ld * es < ((int64_t)1 << 31), "%s: %s view beyond 2 GiB (32-bit DMA offsets)", who, p_name);
  return IMT_OK;
}

}  // namespace
