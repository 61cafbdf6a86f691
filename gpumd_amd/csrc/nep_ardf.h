// Angular-resolved radial distribution function sampled while a run loop owns the state (nepmi_ardf_*, include/nepmi.h): what
// AngularRDF::process / gpu_find_angular_rdf_ON1 accumulate (src/measure/angular_rdf.cu:37-300, :506-583), as an integer histogram
// in the distance r and the azimuth of the pair vector in the xy plane.
//
// Definition.  C columns, 1 <= C <= 7: column 0 "total", then up to six ordered type pairs (a_k, b_k) as the caller lists them;
// R radial bins (1 .. 500), T azimuth bins (1 .. 1024).  An ordered pair i -> j, i != j, has the minimum-image vector
// d = r_j - r_i in double, d2 = |d|^2 and theta = atan2(d_y, d_x); it counts if 0 < d2 <= rc * rc.
//   radial bin   the w with lo_w^2 < d2 <= up_w^2, the edges formed as the reference forms them (angular_rdf.cu:116-118,
//                :459-469): radial[w] = w dr + dr / 2, lo = radial[w] - dr / 2, up = radial[w] + dr / 2, dr = rc / R.  Evaluated
//                as the smallest w with d2 <= up_w^2 (where rounding leaves an ulp between up_w and lo_(w+1) the pair still has one
//                bin); a pair with d2 <= rc * rc above up_(R-1)^2 counts nowhere, as in the reference.
//   azimuth bin  the smallest t with theta <= up_t, clamped to T - 1; up_t = (-PI + t D + D / 2) + D / 2, D = 2 PI / T, formed
//                as at :119-121, :474-478 with the reference's own PI (3.14159265358979, utilities/common.cuh:20).  The direction
//                -x (d_y = 0, d_x < 0) lands in bin T - 1 whatever the sign of its zero; d_x = d_y = 0 is theta = 0.
//   columns      column 0: every ordered pair (an unordered pair adds two counts, at theta and at the reversed direction);
//                (a, a): every ordered pair of two type-a atoms; (a, b), a != b: each unordered a-b pair ONCE, in the direction
//                from the a atom to the b atom (the reference adds that direction from both ends and halves it when it prints,
//                :239-296, :642-644).
// On the device:  counts[C][R][T] unsigned 64-bit;  vsum[C][R][T] double, += (double)count_of_the_sample * volume_of_the_sample
// (the reference normalises with each sample's own volume, :538-543); the sample counter.  Nothing is divided here; the
// normalisation (bv = D / (2 pi) * 4 pi / 3 (up^3 - lo^3); total: vsum / (N^2 bv S), (a, a): vsum / (N_a^2 bv S), (a, b):
// vsum / (N_a N_b bv S)) is the reader's.  Integer sums: exact, independent of the order of atoms and additions, the same bits run
// after run.  No floating-point atomics anywhere.
//
// How the azimuth bin is evaluated (ardf_tbin): no double atan2 on the hit path.  A float atan2f gives an estimate of the bin; it
// is corrected by comparisons in double against a table of the edges' directions (cos up_t, sin up_t): theta <= up_t is the sign
// of the cross product cos(up_t) d_y - sin(up_t) d_x while the two directions are less than half a turn apart, which the estimate
// guarantees.  This is the rule above except for a theta within a few 2^-52 rad of an edge, where the atan2 of two libraries
// differ as well.  The reversed direction -d takes the same path from the estimate turned by pi.
//
// One sample (ArdfT::sample), every launch behind the engine's freeze word: the sequence of nep_rdf.h with its bodies --
//   zero + bin, scan + fill   RdfZeroBody, RdfBinBody, RdfFillBody on cells of edge >= rc / 2 numbered in 4 x 4 x 4 blocks; the
//                             cell starts by the tiled scan of nep_adf.h
//   pairs        nepmi_ardf_pairs below (backends without it, tests/emu: ArdfPlainBody, one work-item per centre atom over the
//                same cell list and the same bin rule)
//   accumulate   RdfAccumBody, one work-item per word: per-sample table -> counts and vsum, table cleared
//
// nepmi_ardf_pairs<LDSHIST>: the frame of nepmi_rdf_pairs -- persistent 256-lane workgroups, grid-stride over the blocks, a
// block's window staged through LDS in chunks of kRdfChunk atoms with the image shift applied, every lane one centre atom in
// registers, an unordered pair taken once from the side that comes first in the cell-sorted order.  A hit forms the r bin from d2
// against the squared edges, both azimuth bins (for d and for -d), and issues two LDS adds for column 0, then per listed column
// two adds for (a, a) when both atoms are a, one add for (a, b) in the a -> b direction.  The table is [C][R][T] 32-bit in LDS,
// flushed to the per-sample global table with 64-bit integer atomics (non-zero words only) when the workgroup is done and before
// the workgroup's count of tested pairs could carry a counter past 2^32 - 1: a hit adds at most 2 to any one word, so the flush
// comes at half of RDF's bound.  When kRdfFixedLds + 4 C R T does not fit in kRdfLdsPerWorkgroup (half a CU's 160 KB) the same
// kernel adds straight to the global table with 64-bit integer atomics.  The rule counts bytes; nothing is timed.
// (36 azimuth bins: total only fits up to 408 radial bins; total + three pairs up to 102.)
//
// Compiled for gfx950 (the compiler's resource line):
//   nepmi_ardf_pairs<true>   82 VGPRs, 106 SGPRs, scratch 0, static LDS 0 (dynamic: kRdfFixedLds + 4 C R T)
//   nepmi_ardf_pairs<false>  80 VGPRs, 106 SGPRs, scratch 0, static LDS 0 (dynamic: kRdfFixedLds)
// (nepmi_rdf_pairs<true> beside them: 70 VGPRs.)
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <type_traits>
#include <vector>

#include "nep_adf.h"
#include "nep_rdf.h"

namespace nepmi {

constexpr int kArdfMaxPairs = 6;
constexpr int kArdfMaxRBins = 500;
constexpr int kArdfMaxTBins = 1024;
constexpr double kArdfPi = 3.14159265358979; // the reference's PI (utilities/common.cuh:20): the edges are formed with it

struct ArdfArgs {
  RdfGrid g;
  double rc2, dr;
  float inv_dr, inv_dt; // 1 / dr, 1 / D
  int R, T, C;
  int zero_bin;                           // the azimuth bin of theta = 0
  int pa[kArdfMaxPairs], pb[kArdfMaxPairs]; // the listed columns' types; unused entries -1
  const double* cs;                       // [T][2]: cos up_t, sin up_t
  const RdfRec* srt;                      // [n] cell-sorted
  const int* cell_start;                  // [64 blocks + 1]
  unsigned long long* table;              // [C][R][T], the sample's own
};

#if defined(__HIP_DEVICE_COMPILE__)
#define NEPMI_ARDF_COUNT(ptr) atomicAdd((ptr), 1ull)
#else
#define NEPMI_ARDF_COUNT(ptr) (void)(++*(ptr))
#endif

// the radial bin of d2, or -1: one estimate, then at most one step against the squared edges -- no loop over bins
NEPMI_HD int ardf_rbin(double d2, double dr, float inv_dr, int R)
{
#pragma clang fp contract(off)
  int w = (int)(sqrtf((float)d2) * inv_dr);
  if (w > R - 1)
    w = R - 1;
  const double half = dr / 2;
  const double up = ((double)w * dr + half) + half;
  if (d2 > up * up) {
    ++w;
  } else if (w > 0) {
    const double below = ((double)(w - 1) * dr + half) + half;
    if (d2 <= below * below)
      --w;
  }
  if (w == 0) { // lo_0 = (0 dr + dr / 2) - dr / 2
    const double lo = half - half;
    if (!(d2 > lo * lo))
      return -1;
  }
  return w < R ? w : -1;
}

// the azimuth bin of the direction (dx, dy); est: its angle to float accuracy
NEPMI_HD int ardf_tbin(const ArdfArgs& a, double dx, double dy, float est)
{
#pragma clang fp contract(off)
  const int T = a.T;
  if (T == 1)
    return 0;
  if (dy == 0.0) {
    if (dx < 0.0)
      return T - 1;
    if (dx == 0.0)
      return a.zero_bin;
  }
  int t = (int)((est + 3.14159265f) * a.inv_dt);
  t = t < 0 ? 0 : (t > T - 1 ? T - 1 : t);
  const double* cs = a.cs;
  while (t < T - 1 && !(cs[2 * t] * dy - cs[2 * t + 1] * dx <= 0.0)) // theta > up_t
    ++t;
  while (t > 0 && cs[2 * t - 2] * dy - cs[2 * t - 1] * dx <= 0.0) // theta <= up_(t-1)
    --t;
  return t;
}

// both azimuth bins of a pair vector: t1 for d, t2 for -d
NEPMI_HD void ardf_tbins(const ArdfArgs& a, double dx, double dy, int& t1, int& t2)
{
  const float est = atan2f((float)dy, (float)dx);
  t1 = ardf_tbin(a, dx, dy, est);
  t2 = ardf_tbin(a, 0.0 - dx, 0.0 - dy, est > 0.0f ? est - 3.14159265f : est + 3.14159265f);
}

// one work-item per centre atom (cell-sorted index) over the +-2 cells around its own; a pair counts from its lower index
struct ArdfPlainBody {
  ArdfArgs a;
  NEPMI_HD void operator()(int64_t i) const
  {
#pragma clang fp contract(off)
    const RdfGrid& g = a.g;
    const RdfRec c = a.srt[i];
    const int blk = c.tag >> 6, loc = c.tag & 63;
    const int cc[3] = {(blk % g.nb[0]) * 4 + (loc & 3), ((blk / g.nb[0]) % g.nb[1]) * 4 + ((loc >> 2) & 3),
                       (blk / (g.nb[0] * g.nb[1])) * 4 + (loc >> 4)};
    for (int oz = -g.reach[2]; oz <= g.reach[2]; ++oz)
      for (int oy = -g.reach[1]; oy <= g.reach[1]; ++oy)
        for (int ox = -g.reach[0]; ox <= g.reach[0]; ++ox) {
          int q[3] = {cc[0] + ox, cc[1] + oy, cc[2] + oz};
          double k[3];
          for (int d = 0; d < 3; ++d) {
            k[d] = 0.0;
            if (q[d] < 0) {
              q[d] += g.nc[d];
              k[d] = -1.0;
            } else if (q[d] >= g.nc[d]) {
              q[d] -= g.nc[d];
              k[d] = 1.0;
            }
          }
          const double sx = k[0] * g.h[0] + k[1] * g.h[1] + k[2] * g.h[2];
          const double sy = k[0] * g.h[3] + k[1] * g.h[4] + k[2] * g.h[5];
          const double sz = k[0] * g.h[6] + k[1] * g.h[7] + k[2] * g.h[8];
          const int id = rdf_cell_id(g, q[0], q[1], q[2]);
          for (int64_t j = a.cell_start[id]; j < a.cell_start[id + 1]; ++j) {
            if (j <= i)
              continue;
            const RdfRec r = a.srt[j];
            const double dx = (r.x + sx) - c.x, dy = (r.y + sy) - c.y, dz = (r.z + sz) - c.z;
            const double d2 = dx * dx + dy * dy + dz * dz;
            if (!(d2 <= a.rc2))
              continue;
            const int w = ardf_rbin(d2, a.dr, a.inv_dr, a.R);
            if (w < 0)
              continue;
            int t1, t2;
            ardf_tbins(a, dx, dy, t1, t2);
            const int64_t row = (int64_t)w * a.T, col = (int64_t)a.R * a.T;
            NEPMI_ARDF_COUNT(&a.table[row + t1]);
            NEPMI_ARDF_COUNT(&a.table[row + t2]);
            for (int m = 0; m < a.C - 1; ++m) {
              const int pa = a.pa[m], pb = a.pb[m];
              unsigned long long* tab = a.table + (m + 1) * col + row;
              if (pa == pb) {
                if (c.type == pa && r.type == pa) {
                  NEPMI_ARDF_COUNT(&tab[t1]);
                  NEPMI_ARDF_COUNT(&tab[t2]);
                }
              } else if (c.type == pa && r.type == pb) {
                NEPMI_ARDF_COUNT(&tab[t1]);
              } else if (c.type == pb && r.type == pa) {
                NEPMI_ARDF_COUNT(&tab[t2]);
              }
            }
          }
        }
  }
};

#if defined(__HIPCC__)
template <bool LDSHIST>
__device__ __forceinline__ void ardf_add(const ArdfArgs& a, unsigned* hist, int idx)
{
  if (LDSHIST)
    atomicAdd(&hist[idx], 1u);
  else
    atomicAdd(&a.table[idx], 1ull);
}

// a staged atom r against the lane's centre (position c, type ct, cell-sorted index ci): the pair counts from the side of the
// lower index, in both directions
template <bool LDSHIST>
__device__ __forceinline__ void ardf_hit(const ArdfArgs& a, unsigned* hist, double d2, const RdfRec& r, double cx, double cy, int ct, int ci)
{
  if (d2 <= a.rc2 && r.tag > ci) {
    const int w = ardf_rbin(d2, a.dr, a.inv_dr, a.R);
    if (w >= 0) {
      int t1, t2;
      ardf_tbins(a, r.x - cx, r.y - cy, t1, t2);
      const int row = w * a.T, col = a.R * a.T;
      ardf_add<LDSHIST>(a, hist, row + t1);
      ardf_add<LDSHIST>(a, hist, row + t2);
      const int jt = r.type;
#pragma unroll
      for (int m = 0; m < kArdfMaxPairs; ++m) {
        if (m < a.C - 1) { // (uniform)
          const int pa = a.pa[m], pb = a.pb[m];
          const int base = (m + 1) * col + row;
          if (pa == pb) {
            if (ct == pa && jt == pa) {
              ardf_add<LDSHIST>(a, hist, base + t1);
              ardf_add<LDSHIST>(a, hist, base + t2);
            }
          } else if (ct == pa && jt == pb) {
            ardf_add<LDSHIST>(a, hist, base + t1);
          } else if (ct == pb && jt == pa) {
            ardf_add<LDSHIST>(a, hist, base + t2);
          }
        }
      }
    }
  }
}

// grid: persistent workgroups of kRdfLanes lanes; dynamic LDS: kRdfFixedLds (+ 4 words when LDSHIST)
template <bool LDSHIST>
__global__ void __launch_bounds__(kRdfLanes) nepmi_ardf_pairs(const ArdfArgs a, const int64_t nblocks, const int words, const int* frozen)
{
  if (frozen && *frozen != 0)
    return;
  extern __shared__ __align__(16) unsigned char ardf_lds[];
  RdfRec* stage = reinterpret_cast<RdfRec*>(ardf_lds);                      // [kRdfChunk]
  int* woff = reinterpret_cast<int*>(ardf_lds + kRdfChunk * sizeof(RdfRec)); // [kRdfMaxWindow + 1 (+ 3)]: first staged slot of a window cell
  int* wbeg = woff + kRdfMaxWindow + 4;                                     // [kRdfMaxWindow]: its first cell-sorted index
  int* wcode = wbeg + kRdfMaxWindow;                                        // [kRdfMaxWindow]: its image shift, 2 bits a direction
  unsigned* hist = reinterpret_cast<unsigned*>(wcode + kRdfMaxWindow);      // [words]
  const RdfGrid& g = a.g;
  const int t = (int)threadIdx.x;
  if (LDSHIST)
    for (int idx = t; idx < words; idx += kRdfLanes)
      hist[idx] = 0;
  unsigned long long tested = 0; // pairs tested since the last flush: a word holds at most twice as many
  for (int64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const int c0 = a.cell_start[blk * 64], c1 = a.cell_start[blk * 64 + 64];
    if (c0 == c1)
      continue;
    const int bc[3] = {(int)(blk % g.nb[0]), (int)((blk / g.nb[0]) % g.nb[1]), (int)(blk / ((int64_t)g.nb[0] * g.nb[1]))};
    int lo[3], nw[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const int last = g.nc[d] - 1 - 4 * bc[d] < 3 ? g.nc[d] - 1 - 4 * bc[d] : 3; // last cell of the block that exists
      lo[d] = -g.reach[d];
      nw[d] = last + g.reach[d] - lo[d] + 1; // <= 8
    }
    const int nwin = nw[0] * nw[1] * nw[2];
    __syncthreads(); // (the tables of the block before are done with)
    for (int w = t; w < kRdfMaxWindow; w += kRdfLanes) {
      int cnt = 0;
      if (w < nwin) {
        int q[3] = {4 * bc[0] + lo[0] + w % nw[0], 4 * bc[1] + lo[1] + (w / nw[0]) % nw[1], 4 * bc[2] + lo[2] + w / (nw[0] * nw[1])};
        int code = 0;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          int k = 1;
          if (q[d] < 0) {
            q[d] += g.nc[d];
            k = 0;
          } else if (q[d] >= g.nc[d]) {
            q[d] -= g.nc[d];
            k = 2;
          }
          code |= k << (2 * d);
        }
        const int id = rdf_cell_id(g, q[0], q[1], q[2]);
        const int beg = a.cell_start[id];
        cnt = a.cell_start[id + 1] - beg;
        wbeg[w] = beg;
        wcode[w] = code;
      }
      woff[w] = cnt;
    }
    __syncthreads();
    if (t < 64) { // exclusive scan of the 512 counts: eight a lane, then across the wavefront
      int loc[8], s = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        loc[k] = s;
        s += woff[8 * t + k];
      }
      int incl = s;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int u = __shfl_up(incl, off, 64);
        if (t >= off)
          incl += u;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k)
        woff[8 * t + k] = incl - s + loc[k];
      if (t == 63)
        woff[kRdfMaxWindow] = incl;
    }
    __syncthreads();
    const int total = woff[kRdfMaxWindow];
    // the block's corner, rounded to float: subtracting it is exact for coordinates of few bits and leaves short numbers
    double org[3];
    {
      const double f[3] = {g.reach[0] ? (double)(4 * bc[0]) / (double)g.nc[0] : 0.0, g.reach[1] ? (double)(4 * bc[1]) / (double)g.nc[1] : 0.0,
                           g.reach[2] ? (double)(4 * bc[2]) / (double)g.nc[2] : 0.0};
#pragma unroll
      for (int d = 0; d < 3; ++d)
        org[d] = (double)(float)(g.h[3 * d] * f[0] + g.h[3 * d + 1] * f[1] + g.h[3 * d + 2] * f[2]);
    }
    for (int q0 = 0; q0 < total; q0 += kRdfChunk) {
      const int m = total - q0 < kRdfChunk ? total - q0 : kRdfChunk;
      __syncthreads(); // (the chunk before is done with)
      for (int s = t; s < m; s += kRdfLanes) {
        const int slot = q0 + s;
        int wl = 0, wh = kRdfMaxWindow - 1;
        while (wl < wh) {
          const int mid = (wl + wh) >> 1;
          if (woff[mid + 1] <= slot)
            wl = mid + 1;
          else
            wh = mid;
        }
        const int j = wbeg[wl] + (slot - woff[wl]);
        RdfRec r = a.srt[j];
        const int code = wcode[wl];
        const double k0 = (double)((code & 3) - 1), k1 = (double)(((code >> 2) & 3) - 1), k2 = (double)(((code >> 4) & 3) - 1);
        {
#pragma clang fp contract(off)
          r.x = (r.x + (k0 * g.h[0] + k1 * g.h[1] + k2 * g.h[2])) - org[0];
          r.y = (r.y + (k0 * g.h[3] + k1 * g.h[4] + k2 * g.h[5])) - org[1];
          r.z = (r.z + (k0 * g.h[6] + k1 * g.h[7] + k2 * g.h[8])) - org[2];
        }
        r.tag = j;
        stage[s] = r;
      }
      __syncthreads();
      for (int p0 = c0; p0 < c1; p0 += kRdfLanes) {
        if (LDSHIST) {
          tested += (unsigned long long)kRdfLanes * (unsigned long long)m;
          if (tested > 0x7FFFFFFFull) { // (two adds a hit may meet in one word)
            rdf_flush(hist, words, a.table, t);
            tested = (unsigned long long)kRdfLanes * (unsigned long long)m;
          }
        }
        const int i = p0 + t;
        double cx = 0.0, cy = 0.0, cz = 0.0;
        int ct = 0, ci = 0x7fffffff; // (a lane without a centre: nothing comes after it)
        if (i < c1) {
          const RdfRec c = a.srt[i];
          cx = c.x - org[0];
          cy = c.y - org[1];
          cz = c.z - org[2];
          ct = c.type;
          ci = i;
        }
        // four staged atoms at a time: the eight LDS reads are issued before the first hit's LDS atomic can order them
        int s = 0;
        for (; s + 4 <= m; s += 4) {
          const RdfRec r0 = stage[s], r1 = stage[s + 1], r2 = stage[s + 2], r3 = stage[s + 3];
          const double d0 = rdf_d2(r0, cx, cy, cz), d1 = rdf_d2(r1, cx, cy, cz), d2 = rdf_d2(r2, cx, cy, cz), d3 = rdf_d2(r3, cx, cy, cz);
          ardf_hit<LDSHIST>(a, hist, d0, r0, cx, cy, ct, ci);
          ardf_hit<LDSHIST>(a, hist, d1, r1, cx, cy, ct, ci);
          ardf_hit<LDSHIST>(a, hist, d2, r2, cx, cy, ct, ci);
          ardf_hit<LDSHIST>(a, hist, d3, r3, cx, cy, ct, ci);
        }
        for (; s < m; ++s) {
          const RdfRec r = stage[s];
          ardf_hit<LDSHIST>(a, hist, rdf_d2(r, cx, cy, cz), r, cx, cy, ct, ci);
        }
      }
    }
  }
  if (LDSHIST)
    rdf_flush(hist, words, a.table, t);
}
#endif // __HIPCC__

template <class B, class = void>
struct BackendHasArdf : std::false_type {};
template <class B>
struct BackendHasArdf<B, std::void_t<decltype(B::kHasArdf)>> : std::integral_constant<bool, B::kHasArdf> {};

// Lifetime: as RdfT -- the object works on a copy of its engine's backend and is destroyed BEFORE the engine.
template <class B>
class ArdfT
{
public:
  ArdfT(const B& be, int64_t n, double rc, int num_r_bins, int num_theta_bins, int64_t interval, const int* type_of_atom, int num_types,
        int num_pairs, const int* pair_types)
    : be_(be), n_(n), interval_(interval), rc_(rc), R_(num_r_bins), T_(num_theta_bins), C_(num_pairs + 1)
  {
    be_.frozen = nullptr;
    if (n < 1 || n > 2000000000)
      throw EngineError{-4, "ardf: bad number of atoms"};
    if (!(rc > 0.0) || !std::isfinite(rc))
      throw EngineError{-4, "ardf: radial cutoff should be positive"};
    if (num_r_bins < 1 || num_r_bins > kArdfMaxRBins)
      throw EngineError{-4, "ardf: number of radial bins should be 1 .. 500"};
    if (num_theta_bins < 1 || num_theta_bins > kArdfMaxTBins)
      throw EngineError{-4, "ardf: number of theta bins should be 1 .. 1024"};
    if (interval < 1)
      throw EngineError{-4, "ardf: sample interval should be positive"};
    if (num_pairs < 0 || num_pairs > kArdfMaxPairs)
      throw EngineError{-4, "ardf: number of type pairs should be 0 .. 6"};
    if (num_types < 1 || num_types > 1024)
      throw EngineError{-4, "ardf: a positive number of types is needed"};
    if (num_pairs > 0 && (!pair_types || !type_of_atom))
      throw EngineError{-4, "ardf: type pairs need pair_types and type_of_atom"};
    for (int m = 0; m < kArdfMaxPairs; ++m)
      pa_[m] = pb_[m] = -1;
    for (int m = 0; m < num_pairs; ++m) {
      pa_[m] = pair_types[2 * m];
      pb_[m] = pair_types[2 * m + 1];
      if (pa_[m] < 0 || pa_[m] >= num_types || pb_[m] < 0 || pb_[m] >= num_types)
        throw EngineError{-4, "ardf: a type pair holds a type outside 0 .. num_types - 1"};
    }
    std::vector<int> type((size_t)n, 0);
    if (type_of_atom)
      for (int64_t i = 0; i < n; ++i) {
        if (type_of_atom[i] < 0 || type_of_atom[i] >= num_types)
          throw EngineError{-4, "ardf: type_of_atom holds a type outside 0 .. num_types - 1"};
        type[(size_t)i] = type_of_atom[i];
      }
    words_ = C_ * R_ * T_; // <= 7 * 500 * 1024
    // the azimuth edges as the reference forms them, and their directions
    const double step = 2 * kArdfPi / T_;
    std::vector<double> cs(2 * (size_t)T_);
    zero_bin_ = T_ - 1;
    for (int t = T_ - 1; t >= 0; --t) {
      const double centre = -kArdfPi + t * step + step / 2;
      const double up = centre + step / 2;
      cs[2 * (size_t)t] = std::cos(up);
      cs[2 * (size_t)t + 1] = std::sin(up);
      if (0.0 <= up)
        zero_bin_ = t;
    }
    try {
      type_ = (int*)dalloc(sizeof(int) * (size_t)n);
      cid_ = (int*)dalloc(sizeof(int) * (size_t)n);
      srt_ = (RdfRec*)dalloc(sizeof(RdfRec) * (size_t)n);
      cs_ = (double*)dalloc(sizeof(double) * 2 * (size_t)T_);
      table_ = (unsigned long long*)dalloc(sizeof(unsigned long long) * (size_t)words_);
      counts_ = (unsigned long long*)dalloc(sizeof(unsigned long long) * (size_t)words_);
      vsum_ = (double*)dalloc(sizeof(double) * (size_t)words_);
      be_.h2d(type_, type.data(), sizeof(int) * (size_t)n);
      be_.h2d(cs_, cs.data(), sizeof(double) * 2 * (size_t)T_);
      be_.memset(table_, 0, sizeof(unsigned long long) * (size_t)words_);
      be_.memset(counts_, 0, sizeof(unsigned long long) * (size_t)words_);
      be_.memset(vsum_, 0, sizeof(double) * (size_t)words_);
      be_.sync(); // (the host arrays above end with this constructor)
    } catch (...) {
      release();
      throw;
    }
  }
  ~ArdfT() { release(); }
  ArdfT(const ArdfT&) = delete;
  ArdfT& operator=(const ArdfT&) = delete;

  void* attached_to = nullptr; // the engine whose run loops sample this handle (EngineT::ardf_attach)
  int64_t n() const { return n_; }
  int64_t num_samples() const { return num_samples_; }
  int num_columns() const { return C_; }
  // the counted rule: 1 = the workgroups' tables live in LDS, 2 = integer atomics straight to the global table
  int form() const { return (int64_t)kRdfFixedLds + 4 * (int64_t)words_ <= lds_budget_ ? 1 : 2; }
  void set_lds_budget(int64_t bytes) { lds_budget_ = std::max<int64_t>(0, std::min<int64_t>(bytes, kRdfLdsPerWorkgroup)); }

  // run loops: the counter rules of CorrelatorT
  bool sample_after(int64_t step) const { return (steps_done_ + step + 1) % interval_ == 0; }
  void advance(int64_t nsteps)
  {
    num_samples_ += (steps_done_ + nsteps) / interval_ - steps_done_ / interval_;
    steps_done_ += nsteps;
  }

  // one sample from pos = [3][N] in the caller's order, or from the engine's internal-order records (posq, perm)
  void sample(const double* pos, const PosQ* posq, const int* perm, int64_t N, const BoxD& box, const int* frozen)
  {
    if (N != n_)
      throw EngineError{-4, "ardf: created for another number of atoms"};
    for (int d = 0; d < 3; ++d)
      if (box.pbc[d] && rc_ > box.thickness[d] / 2.5) // angular_rdf.cu:686-695, against the box of this sample
        throw EngineError{-4, "ardf: The box has a thickness < 2.5 RDF radial cutoffs in a periodic direction."};
    RdfGrid g; // the geometry of RdfT::sample
    for (int k = 0; k < 18; ++k)
      g.h[k] = box.h[k];
    double cells = 1.0;
    for (int d = 0; d < 3; ++d) {
      g.reach[d] = box.pbc[d] ? 2 : 0;
      const double c = box.pbc[d] ? std::floor(box.thickness[d] / (0.5 * rc_)) : 1.0;
      g.nc[d] = (int)std::min(c, 1.0e6);
      g.nb[d] = (g.nc[d] + 3) / 4;
      cells *= 4.0 * g.nb[d];
    }
    if (cells > 1.0e9)
      throw EngineError{-4, "ardf: the box holds too many cells of edge rc / 2"};
    const int64_t nblocks = (int64_t)g.nb[0] * g.nb[1] * g.nb[2], ncell = 64 * nblocks;
    if (ncell > cell_cap_) { // (first use, or a box that has grown: with headroom, so that an NPT run settles at once)
      be_.sync();
      if (cell_count_) {
        be_.free(cell_count_);
        be_.free(cell_fill_);
        be_.free(tile_sums_);
        allocs_.erase(std::remove(allocs_.begin(), allocs_.end(), (void*)cell_count_), allocs_.end());
        allocs_.erase(std::remove(allocs_.begin(), allocs_.end(), (void*)cell_fill_), allocs_.end());
        allocs_.erase(std::remove(allocs_.begin(), allocs_.end(), (void*)tile_sums_), allocs_.end());
        cell_count_ = cell_fill_ = tile_sums_ = nullptr;
        cell_cap_ = 0;
      }
      const int64_t cap = ncell + ncell / 4 + 64;
      cell_count_ = (int*)dalloc(sizeof(int) * (size_t)(cap + 4));
      cell_fill_ = (int*)dalloc(sizeof(int) * (size_t)cap);
      tile_sums_ = (int*)dalloc(sizeof(int) * (size_t)((cap + 1) / kAdfScanTile + 8));
      cell_cap_ = cap;
    }
    const RdfSrc src{pos, posq, perm, type_, n_};
    ArdfArgs a;
    a.g = g;
    a.rc2 = rc_ * rc_;
    a.dr = rc_ / R_;
    a.inv_dr = (float)(1.0 / a.dr);
    a.inv_dt = (float)((double)T_ / (2 * kArdfPi));
    a.R = R_;
    a.T = T_;
    a.C = C_;
    a.zero_bin = zero_bin_;
    for (int m = 0; m < kArdfMaxPairs; ++m) {
      a.pa[m] = pa_[m];
      a.pb[m] = pb_[m];
    }
    a.cs = cs_;
    a.srt = srt_;
    a.cell_start = cell_count_;
    a.table = table_;
    const int f = form();
    be_.frozen = frozen;
    try {
      be_.template launch<256>(kSlotMisc, ncell + 1, RdfZeroBody{cell_count_, cell_fill_, ncell});
      be_.template launch<256>(kSlotMisc, n_, RdfBinBody{g, src, cid_, cell_count_});
      if constexpr (BackendHasArdf<B>::value)
        be_.launch_adf_scan(cell_count_, ncell + 1, tile_sums_);
      else
        be_.template launch<64>(kSlotMisc, 1, RdfScanBody{cell_count_, ncell + 1});
      be_.template launch<256>(kSlotMisc, n_, RdfFillBody{g, src, cid_, cell_count_, cell_fill_, srt_});
      if constexpr (BackendHasArdf<B>::value)
        be_.launch_ardf_pairs(a, nblocks, f == 1, words_);
      else
        be_.template launch<64>(kSlotMisc, n_, ArdfPlainBody{a});
      be_.template launch<256>(kSlotMisc, words_, RdfAccumBody{table_, counts_, vsum_, box.volume});
    } catch (...) {
      be_.frozen = nullptr;
      throw;
    }
    be_.frozen = nullptr;
  }
  void sample_now(const double* pos, const BoxD& box) // nepmi_ardf_sample
  {
    if (!(box.volume > 0.0))
      throw EngineError{-4, "ardf: the box has no volume"};
    sample(pos, nullptr, nullptr, n_, box, nullptr);
    ++num_samples_;
  }
  void read(unsigned long long* counts, double* vsum, int64_t* samples)
  {
    if (counts)
      be_.d2h(counts, counts_, sizeof(unsigned long long) * (size_t)words_);
    if (vsum)
      be_.d2h(vsum, vsum_, sizeof(double) * (size_t)words_);
    if (!counts && !vsum)
      be_.sync();
    if (samples)
      *samples = num_samples_;
  }

private:
  void* dalloc(size_t bytes)
  {
    void* p = be_.alloc(bytes);
    if (!p)
      throw EngineError{-5, "ardf: out of memory"};
    allocs_.push_back(p);
    return p;
  }
  void release()
  {
    if (!allocs_.empty())
      be_.sync();
    for (void* p : allocs_)
      be_.free(p);
    allocs_.clear();
  }

  B be_;
  int64_t n_, interval_;
  double rc_;
  int R_, T_, C_;
  int pa_[kArdfMaxPairs], pb_[kArdfMaxPairs];
  int zero_bin_ = 0;
  int words_ = 0;
  int64_t lds_budget_ = kRdfLdsPerWorkgroup;
  int64_t num_samples_ = 0, steps_done_ = 0;
  int64_t cell_cap_ = 0;
  std::vector<void*> allocs_;
  int* type_ = nullptr;
  int* cid_ = nullptr;
  RdfRec* srt_ = nullptr;
  double* cs_ = nullptr;
  unsigned long long* table_ = nullptr;
  unsigned long long* counts_ = nullptr;
  double* vsum_ = nullptr;
  int* cell_count_ = nullptr;
  int* cell_fill_ = nullptr;
  int* tile_sums_ = nullptr;
};

} // namespace nepmi
