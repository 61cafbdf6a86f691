// Angular distribution function sampled while a run loop owns the state (nepmi_adf_*, include/nepmi.h): what ADF::process /
// gpu_find_adf_global / gpu_find_adf_local accumulate (src/measure/adf.cu:37-176, :237-310), as an integer histogram.
//
// Definition.  A handle holds M <= 32 rows (itype, jtype, ktype, [rmin_j, rmax_j), [rmin_k, rmax_k)); a type of -1 matches any.
// For a centre atom i and a neighbour a != i at the minimum-image distance d2 (double, apply_mic of src/model/box.cuh), a is in
// role J of the row if its type matches jtype and rmin_j^2 <= d2 < rmax_j^2 (closed below, open above: adf.cu:75, :143), in role
// K likewise; a neighbour at d2 == 0 has no direction and is in no role.  The row counts the unordered pair {a, b} once for the
// centre i if type(i) matches itype and (J(a) and K(b)) or (J(b) and K(a)).  The angle: c = (r_ia . r_ib) / sqrt(d2_ia d2_ib)
// clamped to [-1, 1], theta = acos(c) 180 / pi, bin = min(floor(theta / (180 / num_bins)), num_bins - 1) (adf.cu:58-59, :84-91).
// The kernel reaches the bin without acos in double: the neighbours are kept as unit vectors, c is three products and two sums, and the
// bin is looked up in the table ce[b] = cos(b 180 / num_bins degrees) (ce[0] = 1, ce[num_bins] = -1 and, for an even number of
// bins, ce[num_bins / 2] = 0 set exactly): bin b is the one with ce[b + 1] < c <= ce[b] (adf_bin).
//   counts[M][num_bins]  unsigned 64-bit, cumulative over the samples (adf_gpu of the reference is never zeroed either)
// and the sample counter; nothing in floating point, the normalisation is the reader's.
//
// One sample (AdfT::sample), every launch behind the engine's freeze word:
//   zero + bin, scan + fill   the cell binning of nep_rdf.h at rc = the largest rmax of the rows: cells of edge >= rc / 2,
//                             numbered in 4 x 4 x 4 blocks, reach +-2; rc <= thickness / 2.5 is asked at every sample.  The scan
//                             runs in tiles (a short range makes millions of cells: too many for one workgroup)
//   triplets                  nepmi_adf_triplets below (backends without it, tests/emu: AdfPlainBody)
//   accumulate                one work-item per (row, bin): per-sample table -> counts, table cleared; a sample in which a centre
//                             had more than kAdfMaxNeighbours members adds nothing (the overflow word)
//
// nepmi_adf_triplets: persistent workgroups of four wavefronts; a wavefront serves ONE centre atom at a time.
//   phase 1   every lane takes two cells of the centre's +-2 window (at most 125) and walks their atoms from the cell-sorted records;
//             the members of a pass are compacted (ballot + prefix count) into the wavefront's neighbour buffer in LDS: 32 bytes a
//             member, the unit vector in double and two 32-bit masks (role J, role K; one bit per row, only rows whose itype
//             matches the centre).  A candidate with both masks zero is not stored.
//   phase 2   the lanes share the pairs (a < b) of the buffer by their flat index.  The rows hit are (Ja & Kb) | (Jb & Ka); a hit is
//             one adf_bin and one returnless ds_add_u32 per row into the workgroup's LDS table [M][num_bins].
// The table goes to the sample's global table (64-bit integer atomics, non-zero bins only) when the workgroup has finished -- or
// earlier: the workgroup counts the triplets it can have tested since the last flush (a bound on any one 32-bit counter) and
// flushes before that count can pass 2^32 - 1.
// LDS: kAdfBufferLds (four neighbour buffers, 40 KB) + 8 (num_bins + 2) (the table ce) + 4 M num_bins.  Two workgroups share a CU's
// 160 KB, so the LDS table serves while the sum is <= 80 KB; beyond it (32 rows at 720 bins: 90 KB of table) the same kernel adds
// straight into the global table with 64-bit integer atomics.  The rule counts bytes; nothing is timed.
#pragma once
#include "nep_rdf.h"

namespace nepmi {

constexpr int kAdfMaxRows = 32;
constexpr int kAdfLdsPerCu = 160 * 1024;
constexpr int kAdfScanTile = 4096; // cell counts one workgroup of the tiled scan takes
constexpr int kAdfMaxBins = 4096; // (the table ce must fit beside the neighbour buffers)
constexpr int kAdfWaves = 4;
constexpr int kAdfLanes = 64 * kAdfWaves;
// half of a workgroup's LDS share is the four neighbour buffers of 32-byte records
constexpr int kAdfMaxNeighbours = (kRdfLdsPerWorkgroup / 2) / (kAdfWaves * 32);
constexpr int kAdfBufferLds = kAdfWaves * kAdfMaxNeighbours * 32;
static_assert(kAdfMaxNeighbours >= 256, "the neighbour buffer is at least the reference's 200");

struct alignas(16) AdfRec {
  double ux, uy, uz;
  unsigned j, k; // one bit per row: role J, role K
};
static_assert(sizeof(AdfRec) == 32, "a member is 32 bytes");

struct AdfRows {
  int M;
  int it[kAdfMaxRows], jt[kAdfMaxRows], kt[kAdfMaxRows];
  double j0[kAdfMaxRows], j1[kAdfMaxRows], k0[kAdfMaxRows], k1[kAdfMaxRows]; // the SQUARED bounds
};

struct AdfArgs {
  RdfGrid g;
  AdfRows rows;
  double rc2; // the largest squared upper bound
  float inv;  // bins per radian, for the estimate
  int num_bins;
  const double* ce;      // [num_bins + 1]
  const RdfRec* srt;     // [n] cell-sorted
  const int* cell_start; // [64 blocks + 1]
  unsigned long long* table; // [M][num_bins], the sample's own
  int* overflow;             // set when a centre has more than kAdfMaxNeighbours members
};

NEPMI_HD int adf_lds_fixed(int num_bins) { return kAdfBufferLds + 8 * (num_bins + 2); }

// the bin of the cosine c: ce[b + 1] < c <= ce[b]; an estimate in float, then steps against the table
NEPMI_HD int adf_bin(double c, const double* ce, float inv, int num_bins)
{
  c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
  int b = (int)(acosf((float)c) * inv);
  b = b < 0 ? 0 : (b > num_bins - 1 ? num_bins - 1 : b);
  while (b > 0 && c > ce[b])
    --b;
  while (b < num_bins - 1 && !(c > ce[b + 1]))
    ++b;
  return b;
}

// the roles of a neighbour of type t at d2 > 0 around a centre of type ct
NEPMI_HD void adf_masks(const AdfRows& r, int ct, int t, double d2, unsigned& J, unsigned& K)
{
  J = 0;
  K = 0;
  for (int m = 0; m < r.M; ++m) {
    if (r.it[m] >= 0 && r.it[m] != ct)
      continue;
    if ((r.jt[m] < 0 || r.jt[m] == t) && d2 >= r.j0[m] && d2 < r.j1[m])
      J |= 1u << m;
    if ((r.kt[m] < 0 || r.kt[m] == t) && d2 >= r.k0[m] && d2 < r.k1[m])
      K |= 1u << m;
  }
}

// a candidate at the offset (dx, dy, dz) from a centre of type ct: a member's record, or false
NEPMI_HD bool adf_member(const AdfArgs& a, int ct, int t, double dx, double dy, double dz, AdfRec& rec)
{
#pragma clang fp contract(off)
  const double d2 = dx * dx + dy * dy + dz * dz;
  if (!(d2 > 0.0 && d2 < a.rc2))
    return false;
  adf_masks(a.rows, ct, t, d2, rec.j, rec.k);
  if ((rec.j | rec.k) == 0)
    return false;
  const double d = sqrt(d2);
  rec.ux = dx / d;
  rec.uy = dy / d;
  rec.uz = dz / d;
  return true;
}

// three products, two sums, none of them fused: products that cancel (the right angles of a perfect lattice) give exactly 0
NEPMI_HD double adf_cos(const AdfRec& p, const AdfRec& q)
{
#pragma clang fp contract(off)
  return p.ux * q.ux + p.uy * q.uy + p.uz * q.uz;
}

// the cell (cx, cy, cz) of a centre moved by (ox, oy, oz) cells: its id and the periodic image shift of its wrap
NEPMI_HD int adf_window_cell(const RdfGrid& g, const int* cc, int ox, int oy, int oz, double& sx, double& sy, double& sz)
{
#pragma clang fp contract(off)
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
  sx = k[0] * g.h[0] + k[1] * g.h[1] + k[2] * g.h[2];
  sy = k[0] * g.h[3] + k[1] * g.h[4] + k[2] * g.h[5];
  sz = k[0] * g.h[6] + k[1] * g.h[7] + k[2] * g.h[8];
  return rdf_cell_id(g, q[0], q[1], q[2]);
}

NEPMI_HD void adf_cell_of(const RdfGrid& g, int tag, int* cc)
{
  const int blk = tag >> 6, loc = tag & 63;
  cc[0] = (blk % g.nb[0]) * 4 + (loc & 3);
  cc[1] = ((blk / g.nb[0]) % g.nb[1]) * 4 + ((loc >> 2) & 3);
  cc[2] = (blk / (g.nb[0] * g.nb[1])) * 4 + (loc >> 4);
}

// one work-item per centre atom (cell-sorted index) over the +-2 cells around its own: the members into a local array, then the pairs
struct AdfPlainBody {
  AdfArgs a;
  NEPMI_HD void operator()(int64_t i) const
  {
    const RdfGrid& g = a.g;
    const RdfRec c = a.srt[i];
    int cc[3];
    adf_cell_of(g, c.tag, cc);
    AdfRec buf[kAdfMaxNeighbours];
    int m = 0;
    for (int oz = -g.reach[2]; oz <= g.reach[2]; ++oz)
      for (int oy = -g.reach[1]; oy <= g.reach[1]; ++oy)
        for (int ox = -g.reach[0]; ox <= g.reach[0]; ++ox) {
          double sx, sy, sz;
          const int id = adf_window_cell(g, cc, ox, oy, oz, sx, sy, sz);
          for (int64_t j = a.cell_start[id]; j < a.cell_start[id + 1]; ++j) {
            if (j == i)
              continue;
            const RdfRec r = a.srt[j];
            AdfRec rec;
            if (!adf_member(a, c.type, r.type, (r.x + sx) - c.x, (r.y + sy) - c.y, (r.z + sz) - c.z, rec))
              continue;
            if (m == kAdfMaxNeighbours) {
              *a.overflow = 1;
              return;
            }
            buf[m++] = rec;
          }
        }
    for (int q = 1; q < m; ++q)
      for (int p = 0; p < q; ++p) {
        unsigned hit = (buf[p].j & buf[q].k) | (buf[q].j & buf[p].k);
        if (hit == 0)
          continue;
        const int w = adf_bin(adf_cos(buf[p], buf[q]), a.ce, a.inv, a.num_bins);
        for (int row = 0; hit != 0; ++row, hit >>= 1)
          if (hit & 1u)
            NEPMI_RDF_COUNT(&a.table[(int64_t)row * a.num_bins + w]);
      }
  }
};

struct AdfAccumBody {
  unsigned long long* table;
  unsigned long long* counts;
  const int* overflow;
  NEPMI_HD void operator()(int64_t i) const
  {
    const unsigned long long c = table[i];
    table[i] = 0;
    if (c == 0 || *overflow != 0)
      return;
    counts[i] += c;
  }
};

#if defined(__HIPCC__)
// lanes of one wavefront hand data to each other through LDS: order the writes before the reads
#if defined(__HIP_DEVICE_COMPILE__)
#define NEPMI_ADF_WAVE_SYNC()                              \
  do {                                                     \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
    __builtin_amdgcn_wave_barrier();                       \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); \
  } while (0)
#else
#define NEPMI_ADF_WAVE_SYNC() \
  do {                        \
  } while (0)
#endif

// The cell starts of a fine grid (a range of 4 A cuts PbTe's million atoms into 3.5 million cells) are too many for the one
// workgroup of nepmi_rdf_scan: tiles of kAdfScanTile counts are scanned in place by a workgroup each, the tiles' sums by
// nepmi_rdf_scan, and a third pass adds every tile's offset.
__global__ void __launch_bounds__(1024) nepmi_adf_scan_tiles(int* data, const int64_t m, int* tile_sums, const int* frozen)
{
  if (frozen && *frozen != 0)
    return;
  __shared__ int sums[1024];
  const int t = (int)threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * kAdfScanTile + 4 * t;
  int v[4], s = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[k] = base + k < m ? data[base + k] : 0;
    s += v[k];
  }
  sums[t] = s;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int u = t >= off ? sums[t - off] : 0;
    __syncthreads();
    sums[t] += u;
    __syncthreads();
  }
  int run = sums[t] - s;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (base + k < m)
      data[base + k] = run;
    run += v[k];
  }
  if (t == 1023)
    tile_sums[blockIdx.x] = run;
}

__global__ void __launch_bounds__(1024) nepmi_adf_scan_add(int* data, const int64_t m, const int* tile_sums, const int* frozen)
{
  if (frozen && *frozen != 0)
    return;
  const int add = tile_sums[blockIdx.x];
  const int64_t base = (int64_t)blockIdx.x * kAdfScanTile + 4 * (int)threadIdx.x;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (base + k < m)
      data[base + k] += add;
}

__device__ inline void adf_flush(unsigned* hist, int words, unsigned long long* table, int t)
{
  __syncthreads();
  for (int idx = t; idx < words; idx += kAdfLanes) {
    const unsigned v = hist[idx];
    if (v != 0) {
      atomicAdd(&table[idx], (unsigned long long)v);
      hist[idx] = 0;
    }
  }
  __syncthreads();
}

// grid: persistent workgroups of kAdfLanes lanes; dynamic LDS: adf_lds_fixed(num_bins) (+ 4 words when LDSHIST)
template <bool LDSHIST>
__global__ void __launch_bounds__(kAdfLanes) nepmi_adf_triplets(const AdfArgs a, const int64_t n, const int words, const int* frozen)
{
  if (frozen && *frozen != 0)
    return;
  extern __shared__ __align__(16) unsigned char adf_lds[];
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  AdfRec* buf = reinterpret_cast<AdfRec*>(adf_lds) + wave * kAdfMaxNeighbours; // [kAdfMaxNeighbours] of this wavefront
  double* ce = reinterpret_cast<double*>(adf_lds + kAdfBufferLds);             // [num_bins + 1 (+ 1)]
  unsigned* hist = reinterpret_cast<unsigned*>(ce + a.num_bins + 2);           // [words]
  const RdfGrid& g = a.g;
  for (int b = t; b <= a.num_bins; b += kAdfLanes)
    ce[b] = a.ce[b];
  if (LDSHIST)
    for (int idx = t; idx < words; idx += kAdfLanes)
      hist[idx] = 0;
  const int nw[3] = {2 * g.reach[0] + 1, 2 * g.reach[1] + 1, 2 * g.reach[2] + 1};
  const int nwin = nw[0] * nw[1] * nw[2]; // <= 125
  __syncthreads(); // (ce and the cleared table are in place; from here on a wavefront works on its own buffer)
  constexpr unsigned long long kPairsPerPass = (unsigned long long)kAdfWaves * kAdfMaxNeighbours * (kAdfMaxNeighbours - 1) / 2;
  unsigned long long tested = 0; // triplets that can have been tested since the last flush: no 32-bit counter holds more
  for (int64_t base = (int64_t)blockIdx.x * kAdfWaves; base < n; base += (int64_t)gridDim.x * kAdfWaves) {
    if (LDSHIST) {
      tested += kPairsPerPass;
      if (tested > 0xFFFFFFFFull) {
        adf_flush(hist, words, a.table, t);
        tested = kPairsPerPass;
      }
    }
    NEPMI_ADF_WAVE_SYNC(); // (the pair loop of the centre before is done with the buffer)
    const int64_t i = base + wave;
    int m = 0;
    if (i < n) {
      const RdfRec c = a.srt[i];
      int cc[3];
      adf_cell_of(g, c.tag, cc);
      // a lane takes the window cells `lane` and `lane + 64` (at most 125 cells) and walks both at once: two loads in flight
      int beg[2] = {0, 0}, cnt[2] = {0, 0};
      double sx[2] = {0.0, 0.0}, sy[2] = {0.0, 0.0}, sz[2] = {0.0, 0.0};
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int w = lane + 64 * u;
        if (w < nwin) {
          const int id = adf_window_cell(g, cc, w % nw[0] - g.reach[0], (w / nw[0]) % nw[1] - g.reach[1], w / (nw[0] * nw[1]) - g.reach[2],
                                         sx[u], sy[u], sz[u]);
          beg[u] = a.cell_start[id];
          cnt[u] = a.cell_start[id + 1] - beg[u];
        }
      }
      const int cmax = cnt[0] > cnt[1] ? cnt[0] : cnt[1];
      for (int s = 0; __any(s < cmax); ++s) {
        RdfRec r[2];
        bool has[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          has[u] = s < cnt[u] && (int64_t)(beg[u] + s) != i;
          if (has[u])
            r[u] = a.srt[beg[u] + s];
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          AdfRec rec;
          const bool member = has[u] && adf_member(a, c.type, r[u].type, (r[u].x + sx[u]) - c.x, (r[u].y + sy[u]) - c.y, (r[u].z + sz[u]) - c.z, rec);
          const unsigned long long bal = __ballot(member);
          if (member) {
            const int slot = m + __popcll(bal & ((1ull << lane) - 1ull));
            if (slot < kAdfMaxNeighbours)
              buf[slot] = rec;
          }
          m += __popcll(bal);
        }
      }
      if (m > kAdfMaxNeighbours) { // never a write outside the buffer, never a silent undercount: the sample is void
        if (lane == 0)
          atomicExch(a.overflow, 1);
        m = 0;
      }
    }
    NEPMI_ADF_WAVE_SYNC(); // (the members are in place)
    const int npairs = m * (m - 1) / 2;
    int p = lane, q = 1; // the pair (p < q) of the flat index q (q - 1) / 2 + p
    while (p >= q) {
      p -= q;
      ++q;
    }
    for (int f = lane; f < npairs; f += 64) {
      const AdfRec A = buf[p], Bq = buf[q];
      unsigned hit = (A.j & Bq.k) | (Bq.j & A.k);
      if (hit != 0) {
        const int w = adf_bin(adf_cos(A, Bq), ce, a.inv, a.num_bins);
        while (hit != 0) {
          const int row = __ffs(hit) - 1;
          hit &= hit - 1;
          if (LDSHIST)
            atomicAdd(&hist[row * a.num_bins + w], 1u);
          else
            atomicAdd(&a.table[row * a.num_bins + w], 1ull);
        }
      }
      p += 64;
      while (p >= q) {
        p -= q;
        ++q;
      }
    }
  }
  if (LDSHIST)
    adf_flush(hist, words, a.table, t);
}
#endif // __HIPCC__

template <class B, class = void>
struct BackendHasAdf : std::false_type {};
template <class B>
struct BackendHasAdf<B, std::void_t<decltype(B::kHasAdf)>> : std::integral_constant<bool, B::kHasAdf> {};

struct AdfRowIn { // nepmi_adf_row
  int itype, jtype, ktype;
  double rmin_j, rmax_j, rmin_k, rmax_k;
};

// Lifetime: as RdfT -- the object works on a copy of its engine's backend and is destroyed BEFORE the engine.
template <class B>
class AdfT
{
public:
  AdfT(const B& be, int64_t n, int num_bins, int64_t interval, const AdfRowIn* rows, int num_rows, const int* type_of_atom, int num_types)
    : be_(be), n_(n), interval_(interval), num_bins_(num_bins)
  {
    be_.frozen = nullptr;
    if (n < 1 || n > 2000000000)
      throw EngineError{-4, "adf: bad number of atoms"};
    if (num_bins < 1)
      throw EngineError{-4, "adf: number of bins should be positive"};
    if (num_bins > kAdfMaxBins)
      throw EngineError{-4, "adf: more than 4096 bins"};
    if (interval < 1)
      throw EngineError{-4, "adf: sample interval should be positive"};
    if (!rows || num_rows < 1 || num_rows > kAdfMaxRows)
      throw EngineError{-4, "adf: the number of rows should be 1 .. 32"};
    bool typed = false;
    rows_.M = num_rows;
    for (int m = 0; m < num_rows; ++m) {
      const AdfRowIn& r = rows[m];
      const bool any = r.itype == -1 && r.jtype == -1 && r.ktype == -1;
      if (!any) {
        if (r.itype < 0 || r.jtype < 0 || r.ktype < 0)
          throw EngineError{-4, "adf: the types of a row are all -1 (any) or all >= 0"};
        if (r.itype >= num_types || r.jtype >= num_types || r.ktype >= num_types)
          throw EngineError{-4, "adf: a row holds a type outside 0 .. num_types - 1"};
        typed = true;
      }
      if (!(r.rmin_j >= 0.0) || !(r.rmin_k >= 0.0))
        throw EngineError{-4, "adf: minimum radial cutoff should not be negative"};
      if (!(r.rmin_j < r.rmax_j) || !(r.rmin_k < r.rmax_k) || !std::isfinite(r.rmax_j) || !std::isfinite(r.rmax_k))
        throw EngineError{-4, "adf: minimum radial cutoff should be less than maximum radial cutoff"};
      rows_.it[m] = r.itype;
      rows_.jt[m] = r.jtype;
      rows_.kt[m] = r.ktype;
      rows_.j0[m] = r.rmin_j * r.rmin_j;
      rows_.j1[m] = r.rmax_j * r.rmax_j;
      rows_.k0[m] = r.rmin_k * r.rmin_k;
      rows_.k1[m] = r.rmax_k * r.rmax_k;
      rc_ = std::max(rc_, std::max(r.rmax_j, r.rmax_k));
    }
    for (int m = num_rows; m < kAdfMaxRows; ++m) {
      rows_.it[m] = rows_.jt[m] = rows_.kt[m] = 0;
      rows_.j0[m] = rows_.j1[m] = rows_.k0[m] = rows_.k1[m] = 0.0;
    }
    if (typed && (num_types < 1 || !type_of_atom))
      throw EngineError{-4, "adf: type_of_atom and a positive number of types are needed"};
    std::vector<int> type((size_t)n, 0);
    if (type_of_atom)
      for (int64_t i = 0; i < n; ++i) {
        if (type_of_atom[i] < 0 || type_of_atom[i] >= num_types)
          throw EngineError{-4, "adf: type_of_atom holds a type outside 0 .. num_types - 1"};
        type[(size_t)i] = type_of_atom[i];
      }
    words_ = num_rows * num_bins;
    std::vector<double> ce((size_t)num_bins + 1);
    const double pi = 3.14159265358979323846;
    for (int b = 0; b <= num_bins; ++b)
      ce[(size_t)b] = std::cos((double)b * (180.0 / num_bins) * (pi / 180.0));
    ce[0] = 1.0;
    ce[(size_t)num_bins] = -1.0;
    if (num_bins % 2 == 0)
      ce[(size_t)num_bins / 2] = 0.0;
    try {
      type_ = (int*)dalloc(sizeof(int) * (size_t)n);
      cid_ = (int*)dalloc(sizeof(int) * (size_t)n);
      srt_ = (RdfRec*)dalloc(sizeof(RdfRec) * (size_t)n);
      ce_ = (double*)dalloc(sizeof(double) * ((size_t)num_bins + 1));
      table_ = (unsigned long long*)dalloc(sizeof(unsigned long long) * (size_t)words_);
      counts_ = (unsigned long long*)dalloc(sizeof(unsigned long long) * (size_t)words_);
      overflow_ = (int*)dalloc(sizeof(int));
      be_.h2d(type_, type.data(), sizeof(int) * (size_t)n);
      be_.h2d(ce_, ce.data(), sizeof(double) * ((size_t)num_bins + 1));
      be_.memset(table_, 0, sizeof(unsigned long long) * (size_t)words_);
      be_.memset(counts_, 0, sizeof(unsigned long long) * (size_t)words_);
      be_.memset(overflow_, 0, sizeof(int));
      be_.sync(); // (the host arrays above end with this constructor)
    } catch (...) {
      release();
      throw;
    }
  }
  ~AdfT() { release(); }
  AdfT(const AdfT&) = delete;
  AdfT& operator=(const AdfT&) = delete;

  void* attached_to = nullptr; // the engine whose run loops sample this handle (EngineT::adf_attach)
  int64_t n() const { return n_; }
  int64_t num_samples() const { return num_samples_; }
  int num_rows() const { return rows_.M; }
  int num_bins() const { return num_bins_; }
  // the counted rule: 1 = the workgroups' tables live in LDS, 2 = integer atomics straight to the global table
  int form() const { return (int64_t)adf_lds_fixed(num_bins_) + 4 * (int64_t)words_ <= lds_budget_ ? 1 : 2; }
  // (a budget above half a CU's LDS, up to all of it, leaves one workgroup per CU: for running the first form on a large table)
  void set_lds_budget(int64_t bytes) { lds_budget_ = std::max<int64_t>(0, std::min<int64_t>(bytes, kAdfLdsPerCu)); }

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
      throw EngineError{-4, "adf: created for another number of atoms"};
    for (int d = 0; d < 3; ++d)
      if (rc_ > box.thickness[d] / 2.5) // adf.cu:404-413, against the box of this sample
        throw EngineError{-4, "adf: The box has a thickness < 2.5 RDF radial cutoffs in a periodic direction."};
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
      throw EngineError{-4, "adf: the box holds too many cells of edge rc / 2"};
    const int64_t nblocks = (int64_t)g.nb[0] * g.nb[1] * g.nb[2], ncell = 64 * nblocks;
    if (ncell > cell_cap_) {
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
    AdfArgs a;
    a.g = g;
    a.rows = rows_;
    a.rc2 = rc_ * rc_;
    a.inv = (float)((double)num_bins_ / 3.14159265358979323846);
    a.num_bins = num_bins_;
    a.ce = ce_;
    a.srt = srt_;
    a.cell_start = cell_count_;
    a.table = table_;
    a.overflow = overflow_;
    const int f = form();
    be_.frozen = frozen;
    try {
      be_.template launch<256>(kSlotMisc, ncell + 1, RdfZeroBody{cell_count_, cell_fill_, ncell});
      be_.template launch<256>(kSlotMisc, n_, RdfBinBody{g, src, cid_, cell_count_});
      if constexpr (BackendHasAdf<B>::value)
        be_.launch_adf_scan(cell_count_, ncell + 1, tile_sums_);
      else
        be_.template launch<64>(kSlotMisc, 1, RdfScanBody{cell_count_, ncell + 1});
      be_.template launch<256>(kSlotMisc, n_, RdfFillBody{g, src, cid_, cell_count_, cell_fill_, srt_});
      if constexpr (BackendHasAdf<B>::value)
        be_.launch_adf_triplets(a, n_, f == 1, words_);
      else
        be_.template launch<64>(kSlotMisc, n_, AdfPlainBody{a});
      be_.template launch<256>(kSlotMisc, words_, AdfAccumBody{table_, counts_, overflow_});
    } catch (...) {
      be_.frozen = nullptr;
      throw;
    }
    be_.frozen = nullptr;
  }
  void check_overflow() // (synchronises)
  {
    int over = 0;
    be_.d2h(&over, overflow_, sizeof(int));
    if (over != 0)
      throw EngineError{-6, "adf: an atom has more neighbours in range than the capacity of " + std::to_string(kAdfMaxNeighbours) +
                              "; the counts of that sample and of every later one are void"};
  }
  void sample_now(const double* pos, const BoxD& box) // nepmi_adf_sample
  {
    sample(pos, nullptr, nullptr, n_, box, nullptr);
    ++num_samples_;
    check_overflow();
  }
  void read(unsigned long long* counts, int64_t* samples)
  {
    check_overflow();
    if (counts)
      be_.d2h(counts, counts_, sizeof(unsigned long long) * (size_t)words_);
    if (samples)
      *samples = num_samples_;
  }

private:
  void* dalloc(size_t bytes)
  {
    void* p = be_.alloc(bytes);
    if (!p)
      throw EngineError{-5, "adf: out of memory"};
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
  double rc_ = 0.0;
  int num_bins_;
  AdfRows rows_;
  int words_ = 0;
  int64_t lds_budget_ = kRdfLdsPerWorkgroup;
  int64_t num_samples_ = 0, steps_done_ = 0;
  int64_t cell_cap_ = 0;
  std::vector<void*> allocs_;
  int* type_ = nullptr;
  int* cid_ = nullptr;
  RdfRec* srt_ = nullptr;
  double* ce_ = nullptr;
  unsigned long long* table_ = nullptr;
  unsigned long long* counts_ = nullptr;
  int* overflow_ = nullptr;
  int* cell_count_ = nullptr;
  int* cell_fill_ = nullptr;
  int* tile_sums_ = nullptr;
};

} // namespace nepmi
