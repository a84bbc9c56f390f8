// The 256 x 256-tile main loop shared by gemm_xl_kernel (gemm.hip) and the fused scoring kernel (score.hip): tile
// geometry, the paired LDS-DMA issue and the per-wave 128 x 64 tile product.  See gemm.hip for the design notes.
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

}  // namespace
