// Steinhardt bond-orientational order sampled while a run loop owns the state (nepmi_orient_*, include/nepmi.h): what
// OrientOrder::process computes (src/measure/orientorder.cu:637-778: find_neighbor, sort_neighbors :516-565, compute_ql_step1
// :314-399, compute_ql_average :470-514, compute_ql_step2 :401-468), per atom, in double.
//
// Definition.  The members of a centre atom i are the atoms a != i at the minimum-image d2 (double, apply_mic of
// src/model/box.cuh) with 0 < d2 < rc^2; mode nnn keeps, of those, the nnn members smallest in (d2, caller's index) -- and none
// where fewer than nnn lie inside rc.  N_i is the number of members used.  Per member, with d = sqrt(d2), rxy = sqrt(x^2 + y^2),
// c = z / d, s = rxy / d (NOT sqrt(1 - c^2): that loses u / s of absolute accuracy for a bond near the z axis) and
// e^{i phi} = (x + i y) / rxy (1 where rxy < 1e-15, orientorder.cu:352-355):
//   Y_lm = sqrt((2l + 1) / 4 pi (l - m)! / (l + m)!) P_l^m(c) e^{i m phi},  m >= 0, P_m^m = (2m - 1)!! s^m WITHOUT the
//   Condon-Shortley sign (_associated_legendre :275-296, _polar_prefactor :298-312); q_lm(i) = (1 / N_i) sum Y_lm.
// Only m >= 0 is kept; q_{l,-m} = (-1)^m conj(q_lm) (:373-379) where it is needed.  The kernel builds the normalised functions
// directly: Pt_0^0 = sqrt(1 / 4 pi), Pt_m^m = sqrt((2m + 1) / 2m) s Pt_{m-1}^{m-1}, then upward in l,
// Pt_l^m = A_lm (c Pt_{l-1}^m - B_lm Pt_{l-2}^m), A_lm = sqrt((4 l^2 - 1) / (l^2 - m^2)), B_lm = sqrt(((l - 1)^2 - m^2) /
// (4 (l - 1)^2 - 1)): no factorial, no cancellation; the coefficients are a host table (orient_coefficients).
// `average` (Lechner-Dellago, :470-514): qbar_lm(i) = (q_lm(i) + sum_{j in members(i)} q_lm(j)) / (N_i + 1) replaces q_lm(i).
// Columns per atom (:401-468): ql[nd], q_l = sqrt(4 pi / (2l + 1) sum_{m=-l..l} |q_lm|^2); if wl, wl[nd] = sum_{m1, m2}
// CG(l; m1, m2) Re(q_m1 q_m2 conj(q_{m1+m2})) / sqrt(2l + 1), the table CG in the order of _init_clebsch_gordan (:228-259); if
// wlhat, wl (sqrt(4 pi / (2l + 1)) / q_l)^3, and 0 where q_l <= 1e-15.  An atom with N_i = 0 has all columns 0 and q_lm = 0 in its
// neighbours' averages.
//   last[n][ncol]  double, the most recent sample          sum[n][ncol]  double, += last per sample
//   nn[n]          int, the members used                   all in the caller's atom order; and the sample counter.
//
// One sample (OrientT::sample), every launch behind the engine's freeze word:
//   zero + bin, scan + fill   the cell binning of nep_rdf.h at rc with the tiled scan of nep_adf.h; the `type` of a sorted record
//                             is the atom's index in the caller's order (the handle's type array is the identity)
//   qlm                       nepmi_orient_qlm<false> below (backends without it, tests/emu: OrientPlainBody): q_lm -> q1[n][C][2]
//   average (if asked)        nepmi_orient_qlm<true>: the members are searched AGAIN (no stored list: 320 ints per atom would be
//                             1.3 GB at a million atoms) and the rows of q1 gathered into q2
//   columns                   OrientColumnsBody, one work-item per (atom, degree): last, sum, nn; nothing where the overflow word is set
//
// nepmi_orient_qlm: persistent workgroups of four wavefronts; a wavefront serves ONE centre atom at a time.
//   phase 1   as nepmi_adf_triplets: the lanes walk the +-2 window, the members are compacted by ballot into the wavefront's
//             LDS buffer (32 bytes: the offset vector and d2) and index array.  Then every member's rank, the number of members
//             smaller in (d2, index, slot), is counted by the lanes (M^2 comparisons of LDS broadcasts) and ord[rank] = slot
//             written for the ranks kept: the order of the members no longer depends on the order the cells were filled in.
//   phase 2   degree by degree; lane L takes the ranks L, L + 64, ... in rising order and keeps the l + 1 complex partial sums
//             in registers (at most 26 doubles); a butterfly of six shuffles per component adds the lanes' sums in a fixed order;
//             lane 0 writes q_lm and N_i.  <true>: lane k takes component k of the row and adds the members' rows in rank order.
// No floating-point atomics anywhere: the same input gives the same bits, whatever else is attached.
// LDS: 4 x (320 x 32 + 2 x 320 x 4) = 51,200 bytes of buffers + 2,808 of coefficients; two workgroups share a CU.  The
// coefficients are read from LDS at every use (orient_ylm_add).
#pragma once
#include "nep_adf.h"

namespace nepmi {

constexpr int kOrientMaxDegrees = 8;
constexpr int kOrientMaxL = 12;
constexpr int kOrientLd = kOrientMaxL + 1;
constexpr int kOrientWaves = 4;
constexpr int kOrientLanes = 64 * kOrientWaves;
constexpr int kOrientMaxNeighbours = kAdfMaxNeighbours;
constexpr int kOrientCoef = 2 * kOrientLd * kOrientLd + kOrientLd; // A[l][m], B[l][m], D[m]
constexpr double kOrientEps = 1e-15;                                // MY_EPSILON, orientorder.cu:329, :418

struct alignas(16) OrientRec {
  double x, y, z, d2;
};
static_assert(sizeof(OrientRec) == 32, "a member is 32 bytes");

struct OrientArgs {
  RdfGrid g;
  double rc2;
  int mode, nnn; // mode 1: the nnn nearest of the members inside rc
  int nd, C;     // degrees; complex components (m >= 0) of one atom's row
  int deg[kOrientMaxDegrees], off[kOrientMaxDegrees];
  const double* coef;    // [kOrientCoef]
  const RdfRec* srt;     // [n] cell-sorted; .type is the atom's index in the caller's order
  const int* cell_start; // [64 blocks + 1]
  double* q;             // [n][C][2], the caller's order: written by the first pass
  double* qavg;          // [n][C][2]: written by the average pass from q
  int* nn;               // [n] the members used (first pass)
  int* overflow;         // set when a centre has more than kOrientMaxNeighbours members inside rc
};

// A_lm, B_lm and the diagonal factors D_m (D_0 = sqrt(1 / 4 pi)) of the recurrences above
inline void orient_coefficients(double* cf)
{
  for (int k = 0; k < kOrientCoef; ++k)
    cf[k] = 0.0;
  for (int l = 1; l <= kOrientMaxL; ++l)
    for (int m = 0; m < l; ++m) {
      cf[l * kOrientLd + m] = std::sqrt((4.0 * l * l - 1.0) / ((double)l * l - (double)m * m));
      cf[kOrientLd * kOrientLd + l * kOrientLd + m] = std::sqrt((((double)l - 1.0) * (l - 1.0) - (double)m * m) / (4.0 * (l - 1.0) * (l - 1.0) - 1.0));
    }
  cf[2 * kOrientLd * kOrientLd] = std::sqrt(1.0 / (4.0 * 3.14159265358979323846));
  for (int m = 1; m <= kOrientMaxL; ++m)
    cf[2 * kOrientLd * kOrientLd + m] = std::sqrt((2.0 * m + 1.0) / (2.0 * m));
}

// the table CG of every degree of the list, one after the other: for m1 = -l .. l, for m2 with |m1 + m2| <= l in rising order,
// <l m1 l m2 | l m1+m2> by Racah's sum (the order and the formula of _init_clebsch_gordan, orientorder.cu:228-259)
inline void orient_clebsch_gordan(const int* deg, int nd, std::vector<double>& cg, int* cgoff)
{
  double fact[3 * kOrientMaxL + 2];
  fact[0] = 1.0;
  for (int k = 1; k < 3 * kOrientMaxL + 2; ++k)
    fact[k] = fact[k - 1] * k;
  cg.clear();
  for (int il = 0; il < nd; ++il) {
    const int l = deg[il];
    cgoff[il] = (int)cg.size();
    const double common = std::sqrt(fact[l] * fact[l] * fact[l] / fact[3 * l + 1]);
    for (int m1 = -l; m1 <= l; ++m1)
      for (int m2 = std::max(-l, -l - m1); m2 <= std::min(l, l - m1); ++m2) {
        const int m = m1 + m2;
        double sum = 0.0;
        for (int z = std::max(0, std::max(-m1, m2)); z <= std::min(l, std::min(l - m1, l + m2)); ++z)
          sum += ((z & 1) ? -1.0 : 1.0) / (fact[z] * fact[l - z] * fact[l - m1 - z] * fact[l + m2 - z] * fact[m1 + z] * fact[z - m2]);
        const double root = std::sqrt(fact[l + m1] * fact[l - m1] * fact[l + m2] * fact[l - m2] * fact[l + m] * fact[l - m] * (2 * l + 1));
        cg.push_back(sum * common * root);
      }
  }
}

// a candidate at the offset (dx, dy, dz): a member's record, or false
NEPMI_HD bool orient_member(double rc2, double dx, double dy, double dz, OrientRec& rec)
{
#pragma clang fp contract(off)
  const double d2 = dx * dx + dy * dy + dz * dz;
  if (!(d2 > 0.0 && d2 < rc2))
    return false;
  rec.x = dx;
  rec.y = dy;
  rec.z = dz;
  rec.d2 = d2;
  return true;
}

// member p before member q: smaller in (d2, caller's index); the slot only makes the order total
NEPMI_HD bool orient_before(double d2p, int ip, int sp, double d2q, int iq, int sq)
{
  return d2p < d2q || (d2p == d2q && (ip < iq || (ip == iq && sp < sq)));
}

// the members kept of M inside rc
NEPMI_HD int orient_keep(const OrientArgs& a, int M) { return a.mode == 1 ? (M >= a.nnn ? a.nnn : 0) : M; }

// c = z / d, s = rxy / d, e^{i phi} of a member
NEPMI_HD void orient_angles(const OrientRec& r, double& c, double& s, double& er, double& ei)
{
#pragma clang fp contract(off)
  const double d = sqrt(r.d2), rxy = sqrt(r.x * r.x + r.y * r.y);
  c = r.z / d;
  s = rxy / d;
  if (rxy < kOrientEps) {
    er = 1.0;
    ei = 0.0;
  } else {
    er = r.x / rxy;
    ei = r.y / rxy;
  }
}

// adds Y_Lm, m = 0 .. L, of one member to (ar, ai): the diagonal, then upward in l; e^{i m phi} by one complex product per m.
// Register pressure (hipcc -Rpass-analysis=kernel-resource-usage, nepmi_orient_qlm<false>): with the upward loop unrolled the
// kernel takes all 512 registers (one wavefront per SIMD) -- presumably the scheduler gathers the up to 156 coefficient reads ahead of
// the arithmetic; kept as a loop it takes 239 (two per SIMD), no scratch.  The table is read as volatile so that the reads stay where
// they are written (LDS broadcasts) instead of being lifted out of the loop over the members
template <int L>
NEPMI_HD void orient_ylm_add(const volatile double* cf, double c, double s, double er, double ei, double* ar, double* ai)
{
  const volatile double* A = cf;
  const volatile double* Bc = cf + kOrientLd * kOrientLd;
  const volatile double* D = cf + 2 * kOrientLd * kOrientLd;
  double pmm = D[0], cr = 1.0, ci = 0.0;
#pragma unroll
  for (int m = 0; m <= L; ++m) {
    if (m > 0) {
      pmm *= D[m] * s;
      const double tr = cr * er - ci * ei, ti = cr * ei + ci * er;
      cr = tr;
      ci = ti;
    }
    double p = pmm, p1 = pmm, p2 = 0.0;
#pragma unroll 1
    for (int l = m + 1; l <= L; ++l) {
      p = A[l * kOrientLd + m] * (c * p1 - Bc[l * kOrientLd + m] * p2);
      p2 = p1;
      p1 = p;
    }
    ar[m] += p * cr;
    ai[m] += p * ci;
  }
}

#define NEPMI_ORIENT_DISPATCH(l, CALL) \
  switch (l) {                         \
  case 0: CALL(0); break;              \
  case 1: CALL(1); break;              \
  case 2: CALL(2); break;              \
  case 3: CALL(3); break;              \
  case 4: CALL(4); break;              \
  case 5: CALL(5); break;              \
  case 6: CALL(6); break;              \
  case 7: CALL(7); break;              \
  case 8: CALL(8); break;              \
  case 9: CALL(9); break;              \
  case 10: CALL(10); break;            \
  case 11: CALL(11); break;            \
  case 12: CALL(12); break;            \
  default: break;                      \
  }

// one work-item per centre atom (cell-sorted index): the members of the +-2 cells into local arrays, their order, then the sums.
// AVG: the second pass, rows of q gathered into qavg.
template <bool AVG>
struct OrientPlainBody {
  OrientArgs a;
  NEPMI_HD void operator()(int64_t i) const
  {
    const RdfGrid& g = a.g;
    const RdfRec c = a.srt[i];
    int cc[3];
    adf_cell_of(g, c.tag, cc);
    OrientRec buf[kOrientMaxNeighbours];
    int idx[kOrientMaxNeighbours], ord[kOrientMaxNeighbours];
    int M = 0;
    bool over = false;
    for (int oz = -g.reach[2]; oz <= g.reach[2] && !over; ++oz)
      for (int oy = -g.reach[1]; oy <= g.reach[1] && !over; ++oy)
        for (int ox = -g.reach[0]; ox <= g.reach[0] && !over; ++ox) {
          double sx, sy, sz;
          const int id = adf_window_cell(g, cc, ox, oy, oz, sx, sy, sz);
          for (int64_t j = a.cell_start[id]; j < a.cell_start[id + 1]; ++j) {
            if (j == i)
              continue;
            const RdfRec r = a.srt[j];
            OrientRec rec;
            if (!orient_member(a.rc2, (r.x + sx) - c.x, (r.y + sy) - c.y, (r.z + sz) - c.z, rec))
              continue;
            if (M == kOrientMaxNeighbours) {
              over = true;
              break;
            }
            buf[M] = rec;
            idx[M++] = r.type;
          }
        }
    if (over) { // never a silent cut: the sample is void
      *a.overflow = 1;
      M = 0;
    }
    const int keep = orient_keep(a, M);
    for (int p = 0; p < M; ++p) {
      int rank = 0;
      for (int q = 0; q < M; ++q)
        rank += orient_before(buf[q].d2, idx[q], q, buf[p].d2, idx[p], p) ? 1 : 0;
      ord[rank] = p;
    }
    const int64_t row = (int64_t)c.type * a.C * 2;
    if (AVG) {
      for (int k = 0; k < 2 * a.C; ++k) {
        double acc = a.q[row + k];
        for (int r = 0; r < keep; ++r)
          acc += a.q[(int64_t)idx[ord[r]] * a.C * 2 + k];
        a.qavg[row + k] = acc / (double)(keep + 1);
      }
      return;
    }
    a.nn[c.type] = keep;
    for (int il = 0; il < a.nd; ++il) {
      const int l = a.deg[il];
      double ar[kOrientLd], ai[kOrientLd];
      for (int m = 0; m <= l; ++m)
        ar[m] = ai[m] = 0.0;
      for (int r = 0; r < keep; ++r) {
        double ct, st, er, ei;
        orient_angles(buf[ord[r]], ct, st, er, ei);
#define NEPMI_ORIENT_CALL(LL) orient_ylm_add<LL>(a.coef, ct, st, er, ei, ar, ai)
        NEPMI_ORIENT_DISPATCH(l, NEPMI_ORIENT_CALL)
#undef NEPMI_ORIENT_CALL
      }
      const double inv = keep > 0 ? 1.0 / (double)keep : 0.0;
      for (int m = 0; m <= l; ++m) {
        a.q[row + 2 * (a.off[il] + m)] = ar[m] * inv;
        a.q[row + 2 * (a.off[il] + m) + 1] = ai[m] * inv;
      }
    }
  }
};

// one work-item per (atom, degree), the caller's order: q_l, w_l, what_l of the row -> last, sum; the first degree writes nn
struct OrientColumnsBody {
  const double* q; // [n][C][2]
  const int* nn_in;
  const double* cg;
  int cgoff[kOrientMaxDegrees], deg[kOrientMaxDegrees], off[kOrientMaxDegrees];
  int nd, C, ncol, wl, wlhat;
  double* last;
  double* sum;
  int* nn;
  const int* overflow;
  NEPMI_HD void operator()(int64_t w) const
  {
#pragma clang fp contract(off)
    if (*overflow != 0)
      return; // a void sample adds nothing
    const int64_t atom = w / nd;
    const int il = (int)(w - atom * nd);
    const int l = deg[il];
    const double* row = q + (atom * C + off[il]) * 2;
    if (il == 0)
      nn[atom] = nn_in[atom];
    double s2 = row[0] * row[0] + row[1] * row[1];
    for (int m = 1; m <= l; ++m)
      s2 += 2.0 * (row[2 * m] * row[2 * m] + row[2 * m + 1] * row[2 * m + 1]);
    const double pi = 3.14159265358979323846;
    const double f = sqrt(4.0 * pi / (2 * l + 1));
    const double ql = f * sqrt(s2);
    double* out = last + atom * ncol;
    double* acc = sum + atom * ncol;
    out[il] = ql;
    acc[il] += ql;
    if (!wl && !wlhat)
      return;
    double wsum = 0.0;
    int k = cgoff[il];
    for (int m1 = -l; m1 <= l; ++m1) {
      double r1, i1;
      get(row, m1, r1, i1);
      const int lo = -l - m1 > -l ? -l - m1 : -l, hi = l - m1 < l ? l - m1 : l;
      for (int m2 = lo; m2 <= hi; ++m2) {
        double r2, i2, r3, i3;
        get(row, m2, r2, i2);
        get(row, m1 + m2, r3, i3);
        const double pr = r1 * r2 - i1 * i2, pi2 = r1 * i2 + i1 * r2;
        wsum += (pr * r3 + pi2 * i3) * cg[k++];
      }
    }
    const double wv = wsum / sqrt(2 * l + 1.0);
    if (wl) {
      out[nd + il] = wv;
      acc[nd + il] += wv;
    }
    if (wlhat) {
      double hv = 0.0;
      if (ql > kOrientEps) {
        const double t = f / ql;
        hv = wv * (t * t * t);
      }
      out[nd + wl * nd + il] = hv;
      acc[nd + wl * nd + il] += hv;
    }
  }
  // q_lm of either sign of m from the m >= 0 half: q_{l,-m} = (-1)^m conj(q_lm)
  NEPMI_HD static void get(const double* row, int m, double& re, double& im)
  {
    if (m >= 0) {
      re = row[2 * m];
      im = row[2 * m + 1];
    } else {
      const double sg = (m & 1) ? -1.0 : 1.0;
      re = sg * row[-2 * m];
      im = -sg * row[-2 * m + 1];
    }
  }
};

#if defined(__HIPCC__)
// the sums of one degree over the members kept of this wavefront's centre; lane 0 writes the row's components
template <int L>
__device__ inline void orient_degree(const OrientRec* buf, const int* ord, const double* cf, int keep, int lane, double* out)
{
  double ar[L + 1], ai[L + 1];
#pragma unroll
  for (int m = 0; m <= L; ++m)
    ar[m] = ai[m] = 0.0;
  for (int r = lane; r < keep; r += 64) {
    double c, s, er, ei;
    orient_angles(buf[ord[r]], c, s, er, ei);
    orient_ylm_add<L>(cf, c, s, er, ei, ar, ai);
  }
#pragma unroll
  for (int m = 0; m <= L; ++m)
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { // (x + y = y + x: every lane ends with the same sum, in the same order every run)
      ar[m] += __shfl_xor(ar[m], o, 64);
      ai[m] += __shfl_xor(ai[m], o, 64);
    }
  if (lane == 0) {
    const double inv = keep > 0 ? 1.0 / (double)keep : 0.0;
#pragma unroll
    for (int m = 0; m <= L; ++m) {
      out[2 * m] = ar[m] * inv;
      out[2 * m + 1] = ai[m] * inv;
    }
  }
}

// grid: persistent workgroups of kOrientLanes lanes
template <bool AVG>
__global__ void __launch_bounds__(kOrientLanes) nepmi_orient_qlm(const OrientArgs a, const int64_t n, const int* frozen)
{
  if (frozen && *frozen != 0)
    return;
  __shared__ OrientRec lds_buf[kOrientWaves][kOrientMaxNeighbours];
  __shared__ int lds_idx[kOrientWaves][kOrientMaxNeighbours];
  __shared__ int lds_ord[kOrientWaves][kOrientMaxNeighbours];
  __shared__ double cf[kOrientCoef];
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  OrientRec* buf = lds_buf[wave];
  int* idx = lds_idx[wave];
  int* ord = lds_ord[wave];
  const RdfGrid& g = a.g;
  for (int k = t; k < kOrientCoef; k += kOrientLanes)
    cf[k] = a.coef[k];
  const int nw[3] = {2 * g.reach[0] + 1, 2 * g.reach[1] + 1, 2 * g.reach[2] + 1};
  const int nwin = nw[0] * nw[1] * nw[2]; // <= 125
  __syncthreads(); // (the coefficients are in place; from here on a wavefront works on its own buffers)
  for (int64_t base = (int64_t)blockIdx.x * kOrientWaves; base < n; base += (int64_t)gridDim.x * kOrientWaves) {
    NEPMI_ADF_WAVE_SYNC(); // (the centre before is done with the buffers)
    const int64_t i = base + wave;
    if (i >= n)
      continue; // (wave-uniform)
    const RdfRec c = a.srt[i];
    int m = 0;
    {
      int cc[3];
      adf_cell_of(g, c.tag, cc);
      // a lane takes the window cells `lane` and `lane + 64` (at most 125 cells) and walks both at once
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
          OrientRec rec;
          const bool member = has[u] && orient_member(a.rc2, (r[u].x + sx[u]) - c.x, (r[u].y + sy[u]) - c.y, (r[u].z + sz[u]) - c.z, rec);
          const unsigned long long bal = __ballot(member);
          if (member) {
            const int slot = m + __popcll(bal & ((1ull << lane) - 1ull));
            if (slot < kOrientMaxNeighbours) {
              buf[slot] = rec;
              idx[slot] = r[u].type;
            }
          }
          m += __popcll(bal);
        }
      }
      if (m > kOrientMaxNeighbours) { // never a write outside the buffers, never a silent cut: the sample is void
        if (lane == 0)
          atomicExch(a.overflow, 1);
        m = 0;
      }
    }
    NEPMI_ADF_WAVE_SYNC(); // (the members are in place)
    const int keep = orient_keep(a, m);
    for (int p = lane; p < m; p += 64) {
      const double d2p = buf[p].d2;
      const int ip = idx[p];
      int rank = 0;
      for (int q = 0; q < m; ++q)
        rank += orient_before(buf[q].d2, idx[q], q, d2p, ip, p) ? 1 : 0;
      if (rank < keep)
        ord[rank] = p; // (the ranks are a permutation of 0 .. m - 1)
    }
    NEPMI_ADF_WAVE_SYNC(); // (the order is in place)
    const int64_t row = (int64_t)c.type * a.C * 2;
    if (AVG) {
      const double inv = 1.0 / (double)(keep + 1);
      for (int k = lane; k < 2 * a.C; k += 64) {
        double acc = a.q[row + k];
        for (int r = 0; r < keep; ++r)
          acc += a.q[(int64_t)idx[ord[r]] * a.C * 2 + k];
        a.qavg[row + k] = acc * inv;
      }
    } else {
      if (lane == 0)
        a.nn[c.type] = keep;
      for (int il = 0; il < a.nd; ++il) {
        double* out = a.q + row + 2 * a.off[il];
#define NEPMI_ORIENT_CALL(LL) orient_degree<LL>(buf, ord, cf, keep, lane, out)
        NEPMI_ORIENT_DISPATCH(a.deg[il], NEPMI_ORIENT_CALL)
#undef NEPMI_ORIENT_CALL
      }
    }
  }
}
#endif // __HIPCC__

template <class B, class = void>
struct BackendHasOrient : std::false_type {};
template <class B>
struct BackendHasOrient<B, std::void_t<decltype(B::kHasOrient)>> : std::integral_constant<bool, B::kHasOrient> {};

// Lifetime: as AdfT -- the object works on a copy of its engine's backend and is destroyed BEFORE the engine.
template <class B>
class OrientT
{
public:
  OrientT(const B& be, int64_t n, int mode, double rc, int nnn, const int* degrees, int num_degrees, int average, int wl, int wlhat,
          int64_t interval)
    : be_(be), n_(n), interval_(interval), rc_(rc), mode_(mode), nnn_(mode == 1 ? nnn : 0), average_(average != 0), wl_(wl != 0), wlhat_(wlhat != 0)
  {
    be_.frozen = nullptr;
    if (n < 1 || n > 2000000000)
      throw EngineError{-4, "orient: bad number of atoms"};
    if (mode != 0 && mode != 1)
      throw EngineError{-4, "orient: mode should be 0 (cutoff) or 1 (nnn)"};
    if (!(rc > 0.0) || !std::isfinite(rc))
      throw EngineError{-4, "orient: cutoff should be a positive number"};
    if (mode == 1 && nnn < 1)
      throw EngineError{-4, "orient: nnn should be a positive integer"};
    if (!degrees || num_degrees < 1 || num_degrees > kOrientMaxDegrees)
      throw EngineError{-4, "orient: the number of degrees should be 1 .. 8"};
    if (interval < 1)
      throw EngineError{-4, "orient: sample interval should be positive"};
    nd_ = num_degrees;
    C_ = 0;
    for (int k = 0; k < kOrientMaxDegrees; ++k)
      deg_[k] = off_[k] = cgoff_[k] = 0;
    for (int k = 0; k < num_degrees; ++k) {
      if (degrees[k] < 0)
        throw EngineError{-4, "orient: a degree should not be negative"};
      if (degrees[k] > kOrientMaxL)
        throw EngineError{-4, "orient: a degree above 12 is not supported"};
      deg_[k] = degrees[k];
      off_[k] = C_;
      C_ += degrees[k] + 1;
    }
    ncol_ = nd_ * (1 + (wl_ ? 1 : 0) + (wlhat_ ? 1 : 0));
    std::vector<double> cg;
    orient_clebsch_gordan(deg_, nd_, cg, cgoff_);
    double cf[kOrientCoef];
    orient_coefficients(cf);
    std::vector<int> ident((size_t)n);
    for (int64_t i = 0; i < n; ++i)
      ident[(size_t)i] = (int)i;
    const size_t qbytes = sizeof(double) * (size_t)n * (size_t)C_ * 2, colbytes = sizeof(double) * (size_t)n * (size_t)ncol_;
    try {
      type_ = (int*)dalloc(sizeof(int) * (size_t)n);
      cid_ = (int*)dalloc(sizeof(int) * (size_t)n);
      srt_ = (RdfRec*)dalloc(sizeof(RdfRec) * (size_t)n);
      coef_ = (double*)dalloc(sizeof(double) * kOrientCoef);
      cg_ = (double*)dalloc(sizeof(double) * cg.size());
      q_ = (double*)dalloc(qbytes);
      qavg_ = average_ ? (double*)dalloc(qbytes) : nullptr;
      last_ = (double*)dalloc(colbytes);
      sum_ = (double*)dalloc(colbytes);
      nn_tmp_ = (int*)dalloc(sizeof(int) * (size_t)n);
      nn_ = (int*)dalloc(sizeof(int) * (size_t)n);
      overflow_ = (int*)dalloc(sizeof(int));
      be_.h2d(type_, ident.data(), sizeof(int) * (size_t)n);
      be_.h2d(coef_, cf, sizeof(double) * kOrientCoef);
      be_.h2d(cg_, cg.data(), sizeof(double) * cg.size());
      be_.memset(q_, 0, qbytes);
      if (qavg_)
        be_.memset(qavg_, 0, qbytes);
      be_.memset(last_, 0, colbytes);
      be_.memset(sum_, 0, colbytes);
      be_.memset(nn_tmp_, 0, sizeof(int) * (size_t)n);
      be_.memset(nn_, 0, sizeof(int) * (size_t)n);
      be_.memset(overflow_, 0, sizeof(int));
      be_.sync(); // (the host arrays above end with this constructor)
    } catch (...) {
      release();
      throw;
    }
  }
  ~OrientT() { release(); }
  OrientT(const OrientT&) = delete;
  OrientT& operator=(const OrientT&) = delete;

  void* attached_to = nullptr; // the engine whose run loops sample this handle (EngineT::orient_attach)
  int64_t n() const { return n_; }
  int ncol() const { return ncol_; }

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
      throw EngineError{-4, "orient: created for another number of atoms"};
    for (int d = 0; d < 3; ++d)
      if (rc_ > box.thickness[d] / 2.5) // against the box of this sample, as the RDF and ADF handles
        throw EngineError{-4, "orient: The box has a thickness < 2.5 cutoffs in a periodic direction."};
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
      throw EngineError{-4, "orient: the box holds too many cells of edge rc / 2"};
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
    OrientArgs a;
    a.g = g;
    a.rc2 = rc_ * rc_;
    a.mode = mode_;
    a.nnn = nnn_;
    a.nd = nd_;
    a.C = C_;
    for (int k = 0; k < kOrientMaxDegrees; ++k) {
      a.deg[k] = deg_[k];
      a.off[k] = off_[k];
    }
    a.coef = coef_;
    a.srt = srt_;
    a.cell_start = cell_count_;
    a.q = q_;
    a.qavg = qavg_;
    a.nn = nn_tmp_;
    a.overflow = overflow_;
    OrientColumnsBody col;
    col.q = average_ ? qavg_ : q_;
    col.nn_in = nn_tmp_;
    col.cg = cg_;
    for (int k = 0; k < kOrientMaxDegrees; ++k) {
      col.cgoff[k] = cgoff_[k];
      col.deg[k] = deg_[k];
      col.off[k] = off_[k];
    }
    col.nd = nd_;
    col.C = C_;
    col.ncol = ncol_;
    col.wl = wl_ ? 1 : 0;
    col.wlhat = wlhat_ ? 1 : 0;
    col.last = last_;
    col.sum = sum_;
    col.nn = nn_;
    col.overflow = overflow_;
    be_.frozen = frozen;
    try {
      be_.template launch<256>(kSlotMisc, ncell + 1, RdfZeroBody{cell_count_, cell_fill_, ncell});
      be_.template launch<256>(kSlotMisc, n_, RdfBinBody{g, src, cid_, cell_count_});
      if constexpr (BackendHasAdf<B>::value)
        be_.launch_adf_scan(cell_count_, ncell + 1, tile_sums_);
      else
        be_.template launch<64>(kSlotMisc, 1, RdfScanBody{cell_count_, ncell + 1});
      be_.template launch<256>(kSlotMisc, n_, RdfFillBody{g, src, cid_, cell_count_, cell_fill_, srt_});
      if constexpr (BackendHasOrient<B>::value) {
        be_.launch_orient_qlm(a, n_, false);
        if (average_)
          be_.launch_orient_qlm(a, n_, true);
      } else {
        be_.template launch<64>(kSlotMisc, n_, OrientPlainBody<false>{a});
        if (average_)
          be_.template launch<64>(kSlotMisc, n_, OrientPlainBody<true>{a});
      }
      be_.template launch<256>(kSlotMisc, n_ * nd_, col);
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
      throw EngineError{-6, "orient: an atom has more neighbours inside the cutoff than the capacity of " + std::to_string(kOrientMaxNeighbours) +
                              "; that sample and every later one are void"};
  }
  void sample_now(const double* pos, const BoxD& box) // nepmi_orient_sample
  {
    sample(pos, nullptr, nullptr, n_, box, nullptr);
    check_overflow();
    ++num_samples_;
  }
  void read(double* last, double* sum, int* nn, int64_t* samples)
  {
    check_overflow();
    if (last)
      be_.d2h(last, last_, sizeof(double) * (size_t)n_ * (size_t)ncol_);
    if (sum)
      be_.d2h(sum, sum_, sizeof(double) * (size_t)n_ * (size_t)ncol_);
    if (nn)
      be_.d2h(nn, nn_, sizeof(int) * (size_t)n_);
    if (samples)
      *samples = num_samples_;
  }

private:
  void* dalloc(size_t bytes)
  {
    void* p = be_.alloc(bytes);
    if (!p)
      throw EngineError{-5, "orient: out of memory"};
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
  int mode_, nnn_;
  bool average_, wl_, wlhat_;
  int nd_ = 0, C_ = 0, ncol_ = 0;
  int deg_[kOrientMaxDegrees], off_[kOrientMaxDegrees], cgoff_[kOrientMaxDegrees];
  int64_t num_samples_ = 0, steps_done_ = 0;
  int64_t cell_cap_ = 0;
  std::vector<void*> allocs_;
  int* type_ = nullptr;
  int* cid_ = nullptr;
  RdfRec* srt_ = nullptr;
  double* coef_ = nullptr;
  double* cg_ = nullptr;
  double* q_ = nullptr;
  double* qavg_ = nullptr;
  double* last_ = nullptr;
  double* sum_ = nullptr;
  int* nn_tmp_ = nullptr;
  int* nn_ = nullptr;
  int* overflow_ = nullptr;
  int* cell_count_ = nullptr;
  int* cell_fill_ = nullptr;
  int* tile_sums_ = nullptr;
};

} // namespace nepmi
