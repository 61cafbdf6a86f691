// Radial distribution function sampled while a run loop owns the state (nepmi_rdf_*, include/nepmi.h): what RDF::process /
// gpu_find_rdf_ON1 accumulate (src/measure/rdf.cu:37-125, :178-202), as an integer histogram.
//
// Definition (rdf.cu:97-118 with apply_mic of src/model/box.cuh): every unordered pair {i, j}, i != j, at its minimum-image
// distance in double counts if 0 < d2 <= rc * rc, in the bin w with (w dr)^2 < d2 <= ((w + 1) dr)^2, dr = rc / num_bins, the
// edges formed as the reference forms them.  The reference adds 1 / (N rho dV) per ORDERED pair in double with atomicAdd; here
//   counts[P][num_bins]  unsigned 64-bit, P = T (T + 1) / 2 type pairs (a <= b; a outer, b from a: the reference's columns)
//   vsum[P][num_bins]    double, += (double)count_of_the_sample * volume_of_the_sample
// and the normalisation (2 vsum / (N_a^2 dV R) ...) is the reader's.  Integer sums do not depend on the order of the additions:
// the same bits run after run, for any order of the atoms in the input.
//
// One sample (RdfT::sample), every launch behind the engine's freeze word:
//   zero + bin   the atoms of THIS sample are binned in cells of edge >= rc / 2 (the reference's geometry: floor(thickness /
//                (rc / 2)) cells in a periodic direction, one cell in a free one, reach +-2) -- the engine's own cells are cut for
//                the potential and only as fresh as the last list rebuild.  Unwrapped input is wrapped here.  Cells are numbered
//                block by block (4 x 4 x 4 cells, the grid padded with empty cells), so a block's atoms are one contiguous run.
//   scan + fill  cell starts; cell-sorted records (wrapped position in double, type, cell)
//   pairs        nepmi_rdf_pairs below (backends without it, tests/emu: RdfPlainBody, one work-item per centre atom over the same
//                cell list and bin rule)
//   accumulate   one work-item per (type pair, bin): per-sample table -> counts and vsum, table cleared.  No floating-point atomics.
//
// nepmi_rdf_pairs: persistent 256-lane workgroups, grid-stride over the blocks.  A block's window (the block +- 2 cells, <= 8^3
// cells, each with the periodic image shift of its wrap) is staged through LDS in chunks of kRdfChunk atoms in cell-sorted order,
// relative to the block's corner and with the shift applied, so the pair loop carries no minimum image: (an image further than the
// +-2 reach of the centre's own cell is further than rc, because a cell is at least rc / 2 thick, and fails the distance test like
// any other far atom; with thickness >= 2.5 rc every pair has at most one image within rc, and it lies inside the window.)  Every
// lane keeps one centre atom in registers and walks the chunk four atoms at a time -- all lanes read the same LDS address, a broadcast -- and a pair
// counts from the side of the atom that comes first in the cell-sorted order.  A hit is one returnless ds_add_u32 into the
// workgroup's LDS table [P][num_bins]; the table goes to the per-sample global table (64-bit integer atomics, non-zero bins only)
// when the workgroup has finished its blocks -- or earlier: the workgroup counts the pairs it has tested since the last flush
// (lanes x chunk atoms per pass, a bound on any one counter) and flushes before that count can pass 2^32 - 1.
// LDS: kRdfFixedLds (staging + window tables, 22.5 KB) + 4 P num_bins.  Two workgroups share a CU's 160 KB, so the LDS table serves
// while kRdfFixedLds + 4 P num_bins <= 80 KB (two types at 500 bins: 6 KB; seven types at 500 bins: 56 KB); beyond it (sixteen
// types at 500 bins: 272 KB) the same kernel adds straight into the global table with 64-bit integer atomics.  The rule counts
// bytes; nothing is timed.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <type_traits>
#include <vector>

#include "nep_bodies.h"

namespace nepmi {

constexpr int kRdfChunk = 512;      // atoms of one staging chunk (32 bytes each)
constexpr int kRdfMaxWindow = 512;  // cells of a block's window: (4 + 2 * 2)^3
constexpr int kRdfLanes = 256;       // lanes of a workgroup
constexpr int kRdfLanesPerCu = 1024; // persistent workgroups: up to 1,024 lanes per CU of the 256 (fewer where the LDS tables are large)
constexpr int kRdfFixedLds = kRdfChunk * 32 + (kRdfMaxWindow + 4 + 2 * kRdfMaxWindow) * 4;
constexpr int kRdfLdsPerWorkgroup = 80 * 1024;

struct alignas(16) RdfRec {
  double x, y, z;
  int type;
  int tag; // cell-sorted array: the atom's cell; staged in LDS: the atom's index in the cell-sorted array
};

struct RdfGrid {
  double h[18]; // cell (columns a, b, c) and inverse, as BoxD
  int nc[3];    // cells per direction
  int nb[3];    // blocks of 4 cells per direction
  int reach[3]; // 2 in a periodic direction, 0 in a free one
};

struct RdfArgs {
  RdfGrid g;
  double rc2, dr;
  float inv_dr;
  int num_bins, T;
  const RdfRec* srt;     // [n] cell-sorted
  const int* cell_start; // [64 blocks + 1]
  unsigned long long* table; // [P][num_bins], the sample's own
};

#if defined(__HIP_DEVICE_COMPILE__)
#define NEPMI_RDF_COUNT(ptr) atomicAdd((ptr), 1ull)
#else
#define NEPMI_RDF_COUNT(ptr) (void)(++*(ptr))
#endif

// the bin of d2, or -1: one estimate, then at most one step against the squared edges (rdf.cu:102-106) -- no loop over bins
NEPMI_HD int rdf_bin(double d2, double dr, float inv_dr, int num_bins)
{
#pragma clang fp contract(off)
  int w = (int)(sqrtf((float)d2) * inv_dr); // (relative error ~1e-7: 5e-5 of a bin at 500 bins)
  if (w > num_bins - 1)
    w = num_bins - 1;
  const double lo = (double)w * dr;
  if (!(d2 > lo * lo)) {
    --w;
  } else {
    const double up = (double)(w + 1) * dr;
    if (d2 > up * up)
      ++w;
  }
  return (w >= 0 && w < num_bins) ? w : -1; // (d2 = 0 ends at -1; d2 above (num_bins dr)^2 but not above rc * rc ends at num_bins)
}

NEPMI_HD int rdf_pair_row(int t1, int t2, int T) // row of the type pair (a <= b), a outer, b from a
{
  const int a = t1 < t2 ? t1 : t2, b = t1 < t2 ? t2 : t1;
  return a * (2 * T - a + 1) / 2 + (b - a);
}

NEPMI_HD int rdf_cell_id(const RdfGrid& g, int cx, int cy, int cz)
{
  return (((cz >> 2) * g.nb[1] + (cy >> 2)) * g.nb[0] + (cx >> 2)) * 64 + ((cz & 3) * 16 + (cy & 3) * 4 + (cx & 3));
}

// wraps the position into the cell along the periodic directions and returns its cell
NEPMI_HD int rdf_locate(const RdfGrid& g, double& x, double& y, double& z)
{
#pragma clang fp contract(off)
  const double* h = g.h;
  int c[3];
  double fl[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    c[d] = 0;
    fl[d] = 0.0;
    if (g.reach[d] == 0)
      continue;
    double s = h[9 + 3 * d] * x + h[10 + 3 * d] * y + h[11 + 3 * d] * z;
    fl[d] = floor(s);
    s -= fl[d];
    const double v = s * (double)g.nc[d];
    const int k = v < (double)g.nc[d] ? (int)v : g.nc[d] - 1; // (s = 1 by rounding, or not a number: the last cell)
    c[d] = k < 0 ? 0 : k;
  }
  x -= fl[0] * h[0] + fl[1] * h[1] + fl[2] * h[2];
  y -= fl[0] * h[3] + fl[1] * h[4] + fl[2] * h[5];
  z -= fl[0] * h[6] + fl[1] * h[7] + fl[2] * h[8];
  return rdf_cell_id(g, c[0], c[1], c[2]);
}

// where a sample's positions come from: [3][n] in the caller's order (perm == nullptr) or the engine's internal-order records;
// the types are the handle's own, in the caller's order
struct RdfSrc {
  const double* pos;
  const PosQ* posq;
  const int* perm;
  const int* type;
  int64_t n;
  NEPMI_HD void load(int64_t k, double& x, double& y, double& z, int& t) const
  {
    if (posq) {
      const PosQ p = posq[k];
      x = p.x;
      y = p.y;
      z = p.z;
    } else {
      x = pos[k];
      y = pos[n + k];
      z = pos[2 * n + k];
    }
    t = type[perm ? (int64_t)perm[k] : k];
  }
};

struct RdfZeroBody {
  int* cell_count; // [ncell + 1]
  int* cell_fill;  // [ncell]
  int64_t ncell;
  NEPMI_HD void operator()(int64_t i) const
  {
    cell_count[i] = 0;
    if (i < ncell)
      cell_fill[i] = 0;
  }
};

struct RdfBinBody {
  RdfGrid g;
  RdfSrc s;
  int* cid;
  int* cell_count;
  NEPMI_HD void operator()(int64_t k) const
  {
    double x, y, z;
    int t;
    s.load(k, x, y, z, t);
    const int id = rdf_locate(g, x, y, z);
    cid[k] = id;
    NEPMI_ATOMIC_ADD(&cell_count[id], 1);
  }
};

struct RdfScanBody { // backends without the scan kernel: one work-item
  int* data;
  int64_t m;
  NEPMI_HD void operator()(int64_t) const
  {
    int run = 0;
    for (int64_t i = 0; i < m; ++i) {
      const int v = data[i];
      data[i] = run;
      run += v;
    }
  }
};

struct RdfFillBody {
  RdfGrid g;
  RdfSrc s;
  const int* cid;
  const int* cell_start;
  int* cell_fill;
  RdfRec* srt;
  NEPMI_HD void operator()(int64_t k) const
  {
    RdfRec r;
    s.load(k, r.x, r.y, r.z, r.type);
    rdf_locate(g, r.x, r.y, r.z);
    const int id = cid[k];
    r.tag = id;
    srt[cell_start[id] + NEPMI_ATOMIC_ADD(&cell_fill[id], 1)] = r;
  }
};

// one work-item per centre atom (cell-sorted index) over the +-2 cells around its own; a pair counts from its lower index
struct RdfPlainBody {
  RdfArgs a;
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
            const int w = rdf_bin(d2, a.dr, a.inv_dr, a.num_bins);
            if (w >= 0)
              NEPMI_RDF_COUNT(&a.table[(int64_t)rdf_pair_row(c.type, r.type, a.T) * a.num_bins + w]);
          }
        }
  }
};

struct RdfAccumBody {
  unsigned long long* table;
  unsigned long long* counts;
  double* vsum;
  double volume;
  NEPMI_HD void operator()(int64_t i) const
  {
    const unsigned long long c = table[i];
    if (c == 0)
      return;
    counts[i] += c;
    vsum[i] += (double)c * volume;
    table[i] = 0;
  }
};

#if defined(__HIPCC__)
// exclusive scan of data[0 .. m) in place, one workgroup of 1024 lanes, every lane a contiguous run (a multiple of four ints)
__global__ void __launch_bounds__(1024) nepmi_rdf_scan(int* data, const int64_t m, const int* frozen)
{
  if (frozen && *frozen != 0)
    return;
  __shared__ int sums[1024];
  const int t = (int)threadIdx.x;
  const int64_t per = ((m + 1023) / 1024 + 3) / 4 * 4;
  const int64_t b = (int64_t)t * per < m ? (int64_t)t * per : m, e = b + per < m ? b + per : m;
  int s = 0;
  int64_t i = b;
  for (; i + 4 <= e; i += 4) {
    const int4 v = *reinterpret_cast<const int4*>(data + i);
    s += (v.x + v.y) + (v.z + v.w);
  }
  for (; i < e; ++i)
    s += data[i];
  sums[t] = s;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int v = t >= off ? sums[t - off] : 0;
    __syncthreads();
    sums[t] += v;
    __syncthreads();
  }
  int run = sums[t] - s;
  for (i = b; i + 4 <= e; i += 4) {
    int4 v = *reinterpret_cast<const int4*>(data + i);
    int4 o;
    o.x = run;
    o.y = o.x + v.x;
    o.z = o.y + v.y;
    o.w = o.z + v.z;
    run = o.w + v.w;
    *reinterpret_cast<int4*>(data + i) = o;
  }
  for (; i < e; ++i) {
    const int v = data[i];
    data[i] = run;
    run += v;
  }
}

__device__ inline void rdf_flush(unsigned* hist, int words, unsigned long long* table, int t)
{
  __syncthreads();
  for (int idx = t; idx < words; idx += kRdfLanes) {
    const unsigned v = hist[idx];
    if (v != 0) {
      atomicAdd(&table[idx], (unsigned long long)v);
      hist[idx] = 0;
    }
  }
  __syncthreads();
}

__device__ __forceinline__ double rdf_d2(const RdfRec& r, double cx, double cy, double cz)
{
#pragma clang fp contract(off)
  const double dx = r.x - cx, dy = r.y - cy, dz = r.z - cz;
  return dx * dx + dy * dy + dz * dz;
}

// a staged atom r against the lane's centre (type ct, cell-sorted index ci): the pair counts from the side of the lower index
template <bool LDSHIST>
__device__ __forceinline__ void rdf_hit(const RdfArgs& a, unsigned* hist, double d2, const RdfRec& r, int ct, int ci)
{
  if (d2 <= a.rc2 && r.tag > ci) {
    const int w = rdf_bin(d2, a.dr, a.inv_dr, a.num_bins);
    if (w >= 0) {
      const int idx = rdf_pair_row(ct, r.type, a.T) * a.num_bins + w;
      if (LDSHIST)
        atomicAdd(&hist[idx], 1u);
      else
        atomicAdd(&a.table[idx], 1ull);
    }
  }
}

// grid: persistent workgroups of kRdfLanes lanes; dynamic LDS: kRdfFixedLds (+ 4 words when LDSHIST)
template <bool LDSHIST>
__global__ void __launch_bounds__(kRdfLanes) nepmi_rdf_pairs(const RdfArgs a, const int64_t nblocks, const int words, const int* frozen)
{
  if (frozen && *frozen != 0)
    return;
  extern __shared__ __align__(16) unsigned char rdf_lds[];
  RdfRec* stage = reinterpret_cast<RdfRec*>(rdf_lds);                      // [kRdfChunk]
  int* woff = reinterpret_cast<int*>(rdf_lds + kRdfChunk * sizeof(RdfRec)); // [kRdfMaxWindow + 1 (+ 3)]: first staged slot of a window cell
  int* wbeg = woff + kRdfMaxWindow + 4;                                    // [kRdfMaxWindow]: its first cell-sorted index
  int* wcode = wbeg + kRdfMaxWindow;                                       // [kRdfMaxWindow]: its image shift, 2 bits a direction
  unsigned* hist = reinterpret_cast<unsigned*>(wcode + kRdfMaxWindow);     // [words]
  const RdfGrid& g = a.g;
  const int t = (int)threadIdx.x;
  if (LDSHIST)
    for (int idx = t; idx < words; idx += kRdfLanes)
      hist[idx] = 0;
  unsigned long long tested = 0; // pairs tested since the last flush: no 32-bit counter holds more
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
          if (tested > 0xFFFFFFFFull) {
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
          rdf_hit<LDSHIST>(a, hist, d0, r0, ct, ci);
          rdf_hit<LDSHIST>(a, hist, d1, r1, ct, ci);
          rdf_hit<LDSHIST>(a, hist, d2, r2, ct, ci);
          rdf_hit<LDSHIST>(a, hist, d3, r3, ct, ci);
        }
        for (; s < m; ++s) {
          const RdfRec r = stage[s];
          rdf_hit<LDSHIST>(a, hist, rdf_d2(r, cx, cy, cz), r, ct, ci);
        }
      }
    }
  }
  if (LDSHIST)
    rdf_flush(hist, words, a.table, t);
}
#endif // __HIPCC__

template <class B, class = void>
struct BackendHasRdf : std::false_type {};
template <class B>
struct BackendHasRdf<B, std::void_t<decltype(B::kHasRdf)>> : std::integral_constant<bool, B::kHasRdf> {};

// Lifetime: as CorrelatorT -- the object works on a copy of its engine's backend and is destroyed BEFORE the engine.
template <class B>
class RdfT
{
public:
  RdfT(const B& be, int64_t n, double rc, int num_bins, int64_t interval, const int* type_of_atom, int num_types)
    : be_(be), n_(n), interval_(interval), rc_(rc), num_bins_(num_bins), T_(num_types)
  {
    be_.frozen = nullptr;
    if (n < 1 || n > 2000000000)
      throw EngineError{-4, "rdf: bad number of atoms"};
    if (!(rc > 0.0))
      throw EngineError{-4, "rdf: radial cutoff should be positive"};
    if (num_bins < 1)
      throw EngineError{-4, "rdf: number of bins should be positive"};
    if (interval < 1)
      throw EngineError{-4, "rdf: sample interval should be positive"};
    if (num_types < 1 || num_types > 1024 || !type_of_atom)
      throw EngineError{-4, "rdf: type_of_atom and a positive number of types are needed"};
    for (int64_t i = 0; i < n; ++i)
      if (type_of_atom[i] < 0 || type_of_atom[i] >= num_types)
        throw EngineError{-4, "rdf: type_of_atom holds a type outside 0 .. num_types - 1"};
    P_ = num_types * (num_types + 1) / 2;
    if ((int64_t)P_ * num_bins > 0x7fffffff / 4)
      throw EngineError{-4, "rdf: too many type pairs x bins"};
    words_ = P_ * num_bins;
    try {
      type_ = (int*)dalloc(sizeof(int) * (size_t)n);
      cid_ = (int*)dalloc(sizeof(int) * (size_t)n);
      srt_ = (RdfRec*)dalloc(sizeof(RdfRec) * (size_t)n);
      table_ = (unsigned long long*)dalloc(sizeof(unsigned long long) * (size_t)words_);
      counts_ = (unsigned long long*)dalloc(sizeof(unsigned long long) * (size_t)words_);
      vsum_ = (double*)dalloc(sizeof(double) * (size_t)words_);
      be_.h2d(type_, type_of_atom, sizeof(int) * (size_t)n);
      be_.memset(table_, 0, sizeof(unsigned long long) * (size_t)words_);
      be_.memset(counts_, 0, sizeof(unsigned long long) * (size_t)words_);
      be_.memset(vsum_, 0, sizeof(double) * (size_t)words_);
    } catch (...) {
      release();
      throw;
    }
  }
  ~RdfT() { release(); }
  RdfT(const RdfT&) = delete;
  RdfT& operator=(const RdfT&) = delete;

  void* attached_to = nullptr; // the engine whose run loops sample this handle (EngineT::rdf_attach)
  int64_t n() const { return n_; }
  int64_t num_samples() const { return num_samples_; }
  int num_pairs() const { return P_; }
  int num_bins() const { return num_bins_; }
  // the counted rule: 1 = the workgroups' tables live in LDS, 2 = integer atomics straight to the global table
  int form() const { return (int64_t)kRdfFixedLds + 4 * (int64_t)words_ <= lds_budget_ ? 1 : 2; }
  int last_form() const { return last_form_; } // of the last sample taken; 0: none yet
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
      throw EngineError{-4, "rdf: created for another number of atoms"};
    for (int d = 0; d < 3; ++d)
      if (rc_ > box.thickness[d] / 2.5) // rdf.cu:283-292, against the box of this sample
        throw EngineError{-4, "rdf: The box has a thickness < 2.5 RDF radial cutoffs in a periodic direction."};
    RdfGrid g;
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
      throw EngineError{-4, "rdf: the box holds too many cells of edge rc / 2"};
    const int64_t nblocks = (int64_t)g.nb[0] * g.nb[1] * g.nb[2], ncell = 64 * nblocks;
    if (ncell > cell_cap_) { // (first use, or a box that has grown: with headroom, so that an NPT run settles at once)
      be_.sync();
      if (cell_count_) {
        be_.free(cell_count_);
        be_.free(cell_fill_);
        allocs_.erase(std::remove(allocs_.begin(), allocs_.end(), (void*)cell_count_), allocs_.end());
        allocs_.erase(std::remove(allocs_.begin(), allocs_.end(), (void*)cell_fill_), allocs_.end());
        cell_count_ = cell_fill_ = nullptr;
        cell_cap_ = 0;
      }
      const int64_t cap = ncell + ncell / 4 + 64;
      cell_count_ = (int*)dalloc(sizeof(int) * (size_t)(cap + 4));
      cell_fill_ = (int*)dalloc(sizeof(int) * (size_t)cap);
      cell_cap_ = cap;
    }
    const RdfSrc src{pos, posq, perm, type_, n_};
    RdfArgs a;
    a.g = g;
    a.rc2 = rc_ * rc_;
    a.dr = rc_ / num_bins_;
    a.inv_dr = (float)(1.0 / a.dr);
    a.num_bins = num_bins_;
    a.T = T_;
    a.srt = srt_;
    a.cell_start = cell_count_;
    a.table = table_;
    const int f = form();
    be_.frozen = frozen;
    try {
      be_.template launch<256>(kSlotMisc, ncell + 1, RdfZeroBody{cell_count_, cell_fill_, ncell});
      be_.template launch<256>(kSlotMisc, n_, RdfBinBody{g, src, cid_, cell_count_});
      if constexpr (BackendHasRdf<B>::value)
        be_.launch_rdf_scan(cell_count_, ncell + 1);
      else
        be_.template launch<64>(kSlotMisc, 1, RdfScanBody{cell_count_, ncell + 1});
      be_.template launch<256>(kSlotMisc, n_, RdfFillBody{g, src, cid_, cell_count_, cell_fill_, srt_});
      if constexpr (BackendHasRdf<B>::value)
        be_.launch_rdf_pairs(a, nblocks, f == 1, words_);
      else
        be_.template launch<64>(kSlotMisc, n_, RdfPlainBody{a});
      be_.template launch<256>(kSlotMisc, words_, RdfAccumBody{table_, counts_, vsum_, box.volume});
    } catch (...) {
      be_.frozen = nullptr;
      throw;
    }
    be_.frozen = nullptr;
    last_form_ = f;
  }
  void sample_now(const double* pos, const BoxD& box) // nepmi_rdf_sample
  {
    if (!(box.volume > 0.0))
      throw EngineError{-4, "rdf: the box has no volume"};
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
      throw EngineError{-5, "rdf: out of memory"};
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
  int num_bins_, T_;
  int P_ = 0, words_ = 0;
  int64_t lds_budget_ = kRdfLdsPerWorkgroup;
  int last_form_ = 0;
  int64_t num_samples_ = 0, steps_done_ = 0;
  int64_t cell_cap_ = 0;
  std::vector<void*> allocs_;
  int* type_ = nullptr;
  int* cid_ = nullptr;
  RdfRec* srt_ = nullptr;
  unsigned long long* table_ = nullptr;
  unsigned long long* counts_ = nullptr;
  double* vsum_ = nullptr;
  int* cell_count_ = nullptr;
  int* cell_fill_ = nullptr;
};

} // namespace nepmi
