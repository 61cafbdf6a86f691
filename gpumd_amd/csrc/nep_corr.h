// Time-correlation sums of per-atom vectors, sampled while a run loop owns the state (nepmi_corr_*, include/nepmi.h):
//   quantity 0 (MSD): sum_i (u_i(t) - u_i(t - l))^2 per component, on unwrapped positions  -- MSD::process, src/measure/msd.cu:269-362
//   quantity 1 (VAC): sum_i  v_i(t) * v_i(t - l)    per component                         -- SDC::process, src/measure/sdc.cu:157-224
//   quantity 2 (MVAC): sum_i (w_i * v_i(t)) * v_i(t - l) per component, w_i a weight per atom (the mass)
//                                                                                        -- gpu_find_vac, src/measure/dos.cu:84-143
// with the reference's bookkeeping: sample s goes to slot s % num_corr of a ring of frames, and from s >= num_corr - 1 on every
// sample is a time origin that adds, for each lag l, the current frame against the one in slot (s - l) mod num_corr.  The
// normalisation (1 / (atoms * origins)) is the reader's.
//
// The weights of quantity 2 are kept in the ring's order, zero in the gaps, and are multiplied into the current frame once per
// sample -- not per lag -- so the walk over the lags is that of quantity 1.  nepmi_dos_from_mvac (capi_impl.h) turns the sums into
// the normalised MVAC and the density of states.
//
// The ring keeps its OWN atom order -- sorted by group, then by the caller's index, every group starting at an even index (the gap
// is a slot nobody writes: zero in every frame, so it adds (0 - 0)^2 or 0 * 0) -- so that
//   - a list rebuild, which changes the engine's internal order, does not touch it: the gather of a sample writes
//     frame[order_of[perm[k]]] = q[k] from whatever the internal order is at that step;
//   - a group is a contiguous range: all atoms, one group and all groups are the same kernel over a table of tiles that are cut at
//     the group boundaries;
//   - every read of the correlation kernel is unit-stride and 16-byte aligned.
//
// The reference launches one 128-thread block per lag, each streaming a whole frame and ending in one thread's `+=`
// (msd.cu:89-149, sdc.cu:71-128).  Here one launch covers all lags: a workgroup takes a tile of 512 atoms x a chunk of lags, keeps
// its part of the current frame in registers while it walks the lags, reduces across the lanes of a wavefront by cross-lane moves
// and across the four wavefronts in LDS, and writes one partial sum per (tile, lag, component).  A second small kernel adds the
// partial sums of a group's tiles to the accumulators in a fixed order: no floating-point atomics, the same bits run after run.
// The lag chunk is chosen so that small systems still fill the device (Correlator: kTargetWorkgroups).
//
// Backends without the kernel (tests/emu: absence of B::kHasCorr means "no") run CorrPlainBody through `launch`: the same ring, lag
// mapping and tile table, one work-item per (group, lag, component).
#pragma once
#include <algorithm>
#include <type_traits>
#include <vector>

#include "nep_bodies.h"

namespace nepmi {

constexpr int kCorrTileAtoms = 512; // 256 lanes x two atoms (one 16-byte load per component)
constexpr int kCorrMaxLagChunk = 64; // lags of one workgroup (bounds its LDS: 4 waves x 3 x 64 doubles)

struct CorrTile {
  int start; // first ring index (even)
  int count; // atoms of the tile, 1 .. kCorrTileAtoms
};

struct CorrArgs {
  const double* ring; // [num_corr][3][ns]
  int64_t ns;         // ring indices per component (even; selected atoms + the gaps in front of odd group starts)
  int num_corr, cur;  // cur: the slot of the frame just taken
  int quantity;
  const CorrTile* tiles;
  const int* tile_first; // [num_groups + 1]: the tiles of group g are tile_first[g] .. tile_first[g + 1] - 1
  int num_tiles, num_groups;
  int lag_chunk, num_chunks;
  double* partial; // [num_corr * 3][num_tiles]
  double* acc;     // [num_groups][3][num_corr]
  const double* weight; // [ns], quantity 2 only: the per-atom weights in the ring's order, zero in the gaps
};

// frame[d][order_of[i]] = q[d][k], i = perm[k] (internal order) or k (caller's order, perm == nullptr)
struct CorrGatherBody {
  const double* q;
  int64_t N;
  const int* perm;
  const int* order_of;
  double* frame;
  int64_t ns;
  NEPMI_HD void operator()(int64_t k) const
  {
    const int64_t i = perm ? (int64_t)perm[k] : k;
    const int j = order_of[i];
    if (j < 0)
      return;
#pragma unroll
    for (int d = 0; d < 3; ++d)
      frame[d * ns + j] = q[d * N + k];
  }
};

struct CorrPlainBody {
  CorrArgs a;
  NEPMI_HD void operator()(int64_t idx) const
  {
    const int per_group = 3 * a.num_corr;
    const int g = (int)(idx / per_group), r = (int)(idx % per_group);
    const int lag = r / 3, d = r % 3;
    int old = a.cur - lag;
    if (old < 0)
      old += a.num_corr;
    const double* c = a.ring + ((int64_t)a.cur * 3 + d) * a.ns;
    const double* o = a.ring + ((int64_t)old * 3 + d) * a.ns;
    double sum = 0.0;
    for (int t = a.tile_first[g]; t < a.tile_first[g + 1]; ++t) {
      const CorrTile T = a.tiles[t];
      double s = 0.0;
      for (int j = T.start; j < T.start + T.count; ++j) {
        if (a.quantity == 0) {
          const double dx = c[j] - o[j];
          s += dx * dx;
        } else if (a.quantity == 2) {
          s += (a.weight[j] * c[j]) * o[j];
        } else {
          s += c[j] * o[j];
        }
      }
      sum += s;
    }
    a.acc[((int64_t)g * 3 + d) * a.num_corr + lag] += sum;
  }
};

#if defined(__HIPCC__)
// wavefront sum by cross-lane moves; lane 0 holds the result
__device__ inline double corr_wave_sum(double v)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    v += __shfl_down(v, off, 64);
  return v;
}

// grid: num_tiles x num_chunks workgroups of 256 lanes
template <int Q>
__global__ void __launch_bounds__(256) nepmi_corr_tiles(const CorrArgs a, const int* frozen)
{
  if (frozen && *frozen != 0)
    return;
  __shared__ double red[4][3 * kCorrMaxLagChunk];
  const int tile = (int)(blockIdx.x / (unsigned)a.num_chunks), chunk = (int)(blockIdx.x % (unsigned)a.num_chunks);
  const CorrTile T = a.tiles[tile];
  const int t = (int)threadIdx.x, wave = t >> 6, lane = t & 63;
  const bool on = 2 * t < T.count; // (an odd count: the pair's second index is the gap behind the group, zero in every frame)
  const int64_t j = (int64_t)T.start + 2 * t;
  double2 c[3] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
  if (on) {
#pragma unroll
    for (int d = 0; d < 3; ++d)
      c[d] = *reinterpret_cast<const double2*>(a.ring + ((int64_t)a.cur * 3 + d) * a.ns + j);
    if (Q == 2) { // the weights go into the current frame: once per sample, and the lags below are those of Q == 1
      const double2 w = *reinterpret_cast<const double2*>(a.weight + j);
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        c[d].x *= w.x;
        c[d].y *= w.y;
      }
    }
  }
  const int l0 = chunk * a.lag_chunk;
  const int l1 = l0 + a.lag_chunk < a.num_corr ? l0 + a.lag_chunk : a.num_corr;
#pragma unroll 2
  for (int l = l0; l < l1; ++l) {
    int old = a.cur - l;
    if (old < 0)
      old += a.num_corr;
    double s[3] = {0.0, 0.0, 0.0};
    if (on) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const double2 o = *reinterpret_cast<const double2*>(a.ring + ((int64_t)old * 3 + d) * a.ns + j);
        if (Q == 0) {
          const double dx = c[d].x - o.x, dy = c[d].y - o.y;
          s[d] = dx * dx + dy * dy;
        } else {
          s[d] = c[d].x * o.x + c[d].y * o.y;
        }
      }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const double w = corr_wave_sum(s[d]);
      if (lane == 0)
        red[wave][(l - l0) * 3 + d] = w;
    }
  }
  __syncthreads();
  if (t < (l1 - l0) * 3) {
    const double sum = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
    a.partial[(int64_t)(l0 * 3 + t) * a.num_tiles + tile] = sum;
  }
}

// grid: num_groups x num_corr x 3 wavefronts: the partial sums of a group's tiles, lane by lane in tile order, then across the lanes
__global__ void __launch_bounds__(64) nepmi_corr_reduce(const CorrArgs a, const int* frozen)
{
  if (frozen && *frozen != 0)
    return;
  const int per_group = 3 * a.num_corr;
  const int g = (int)(blockIdx.x / (unsigned)per_group), r = (int)(blockIdx.x % (unsigned)per_group);
  const int lag = r / 3, d = r % 3;
  const int t1 = a.tile_first[g + 1];
  double s = 0.0;
  for (int t = a.tile_first[g] + (int)threadIdx.x; t < t1; t += 64)
    s += a.partial[(int64_t)r * a.num_tiles + t];
  s = corr_wave_sum(s);
  if (threadIdx.x == 0)
    a.acc[((int64_t)g * 3 + d) * a.num_corr + lag] += s;
}
#endif // __HIPCC__

template <class B, class = void>
struct BackendHasCorr : std::false_type {};
template <class B>
struct BackendHasCorr<B, std::void_t<decltype(B::kHasCorr)>> : std::integral_constant<bool, B::kHasCorr> {};

// Lifetime: the object works on a copy of its engine's backend (stream, staging buffers): it is destroyed BEFORE the engine.
template <class B>
class CorrelatorT
{
public:
  static constexpr int kTargetWorkgroups = 1024; // 4 per CU of the 256: 13,824 atoms x 100 lags are 27 tiles x 34 chunks, not 27 workgroups

  // weight: HOST [n] in the caller's order, for quantity 2 and for it only (nepmi_corr_create_weighted)
  CorrelatorT(const B& be, int quantity, int64_t n, int64_t interval, int num_corr, const int* group_of_atom, int num_groups,
              const double* weight = nullptr)
    : be_(be), quantity_(quantity), n_(n), interval_(interval), num_corr_(num_corr), num_groups_(num_groups)
  {
    be_.frozen = nullptr;
    if (!weight && quantity != 0 && quantity != 1)
      throw EngineError{-4, "correlator: quantity should be 0 (MSD) or 1 (VAC)"};
    if (weight && quantity != 2)
      throw EngineError{-4, "correlator: weights belong to quantity 2 (MVAC)"};
    if (n < 1 || n > 2000000000)
      throw EngineError{-4, "correlator: bad number of atoms"};
    if (interval < 1 || num_corr < 1 || num_groups < 1)
      throw EngineError{-4, "correlator: sample interval, number of correlation steps and number of groups should be positive"};
    // ring order: by group, then by the caller's index; every group starts at an even ring index
    std::vector<int64_t> count((size_t)num_groups, 0);
    for (int64_t i = 0; i < n; ++i) {
      const int g = group_of_atom ? group_of_atom[i] : 0;
      if (g >= num_groups || g < -1)
        throw EngineError{-4, "correlator: group_of_atom holds a group outside -1 .. num_groups - 1"};
      if (g >= 0)
        ++count[g];
    }
    std::vector<int64_t> first((size_t)num_groups + 1, 0);
    for (int g = 0; g < num_groups; ++g)
      first[g + 1] = (first[g] + count[g] + 1) / 2 * 2;
    ns_ = first[num_groups];
    if (ns_ > 2000000000)
      throw EngineError{-4, "correlator: too many atoms"};
    std::vector<int> order((size_t)n, -1);
    {
      std::vector<int64_t> next(first.begin(), first.end() - 1);
      for (int64_t i = 0; i < n; ++i) {
        const int g = group_of_atom ? group_of_atom[i] : 0;
        if (g >= 0)
          order[i] = (int)next[g]++;
      }
    }
    std::vector<CorrTile> tiles;
    std::vector<int> tile_first((size_t)num_groups + 1, 0);
    for (int g = 0; g < num_groups; ++g) {
      tile_first[g] = (int)tiles.size();
      for (int64_t s = 0; s < count[g]; s += kCorrTileAtoms)
        tiles.push_back(CorrTile{(int)(first[g] + s), (int)std::min<int64_t>(kCorrTileAtoms, count[g] - s)});
    }
    tile_first[num_groups] = (int)tiles.size();
    num_tiles_ = (int)tiles.size();
    std::vector<double> w_ring;
    if (weight) {
      w_ring.assign((size_t)std::max<int64_t>(ns_, 2), 0.0); // (the gaps: zero)
      for (int64_t i = 0; i < n; ++i) {
        if (!(weight[i] >= 0.0) || !(weight[i] <= 1.7976931348623157e308)) // (NaN fails both)
          throw EngineError{-4, "correlator: weight should be finite and not negative"};
        if (order[i] >= 0)
          w_ring[(size_t)order[i]] = weight[i];
      }
    }
    // lags per workgroup: all of them where the tiles alone fill the device, fewer where they do not
    int chunks = num_tiles_ > 0 ? (kTargetWorkgroups + num_tiles_ - 1) / num_tiles_ : 1;
    chunks = std::max(chunks, (num_corr + kCorrMaxLagChunk - 1) / kCorrMaxLagChunk);
    chunks = std::min(chunks, num_corr);
    lag_chunk_ = (num_corr + chunks - 1) / chunks;
    num_chunks_ = (num_corr + lag_chunk_ - 1) / lag_chunk_;
    try {
      const size_t ring_doubles = (size_t)num_corr * 3 * (size_t)std::max<int64_t>(ns_, 2);
      ring_ = (double*)dalloc(sizeof(double) * ring_doubles);
      acc_ = (double*)dalloc(sizeof(double) * (size_t)num_groups * 3 * num_corr);
      order_of_ = (int*)dalloc(sizeof(int) * (size_t)n);
      tiles_ = (CorrTile*)dalloc(sizeof(CorrTile) * std::max<size_t>(tiles.size(), 1));
      tile_first_ = (int*)dalloc(sizeof(int) * tile_first.size());
      partial_ = (double*)dalloc(sizeof(double) * (size_t)num_corr * 3 * (size_t)std::max(num_tiles_, 1));
      be_.memset(ring_, 0, sizeof(double) * ring_doubles); // (the gaps stay zero for good)
      be_.memset(acc_, 0, sizeof(double) * (size_t)num_groups * 3 * num_corr);
      be_.h2d(order_of_, order.data(), sizeof(int) * (size_t)n);
      if (!tiles.empty())
        be_.h2d(tiles_, tiles.data(), sizeof(CorrTile) * tiles.size());
      be_.h2d(tile_first_, tile_first.data(), sizeof(int) * tile_first.size());
      if (weight) {
        weight_ = (double*)dalloc(sizeof(double) * w_ring.size());
        be_.h2d(weight_, w_ring.data(), sizeof(double) * w_ring.size());
      }
    } catch (...) {
      release();
      throw;
    }
  }
  ~CorrelatorT() { release(); }
  CorrelatorT(const CorrelatorT&) = delete;
  CorrelatorT& operator=(const CorrelatorT&) = delete;

  void* attached_to = nullptr; // the engine whose run loops sample this correlator (EngineT::corr_attach)
  int quantity() const { return quantity_; }
  bool samples_velocities() const { return quantity_ != 0; } // VAC and MVAC: the second half-kick of a sample step cannot wait
  int64_t n() const { return n_; }
  int64_t num_samples() const { return num_samples_; }
  int64_t num_origins() const { return std::max<int64_t>(0, num_samples_ - (num_corr_ - 1)); }

  // Run loops: everything about the sample behind step `step` (0-based) of the current call is a function of the counters at the
  // call's entry and of `step` -- a step that is replayed after a rebuild takes the same slot, lags and origin count again.
  int64_t sample_index_after(int64_t step) const // -1: not a sample step
  {
    const int64_t t = steps_done_ + step + 1;
    if (t % interval_ != 0)
      return -1;
    return num_samples_ + (t / interval_ - steps_done_ / interval_) - 1;
  }
  void advance(int64_t nsteps) // the call has ended: nsteps steps stand
  {
    num_samples_ += (steps_done_ + nsteps) / interval_ - steps_done_ / interval_;
    steps_done_ += nsteps;
  }

  // sample number s from q = [3][N] in the order of perm (nullptr: the caller's); every kernel returns at once when *frozen != 0
  void sample(const double* q, int64_t N, const int* perm, int64_t s, const int* frozen)
  {
    if (N != n_)
      throw EngineError{-4, "correlator: created for another number of atoms"};
    if (ns_ == 0)
      return;
    const int cur = (int)(s % num_corr_);
    be_.frozen = frozen;
    try {
      be_.template launch<256>(kSlotMisc, N, CorrGatherBody{q, N, perm, order_of_, ring_ + (int64_t)cur * 3 * ns_, ns_});
      if (s >= num_corr_ - 1) {
        const CorrArgs a{ring_, ns_, num_corr_, cur, quantity_, tiles_, tile_first_, num_tiles_, num_groups_, lag_chunk_, num_chunks_,
                         partial_, acc_, weight_};
        if constexpr (BackendHasCorr<B>::value)
          be_.launch_corr(a);
        else
          be_.template launch<64>(kSlotMisc, (int64_t)num_groups_ * 3 * num_corr_, CorrPlainBody{a});
      }
    } catch (...) {
      be_.frozen = nullptr;
      throw;
    }
    be_.frozen = nullptr;
  }
  void sample_now(const double* q) // nepmi_corr_sample: the next sample, from the caller's order
  {
    sample(q, n_, nullptr, num_samples_, nullptr);
    ++num_samples_;
  }
  void read(double* sums, int64_t* origins, int64_t* samples)
  {
    if (sums)
      be_.d2h(sums, acc_, sizeof(double) * (size_t)num_groups_ * 3 * num_corr_);
    else
      be_.sync();
    if (origins)
      *origins = num_origins();
    if (samples)
      *samples = num_samples_;
  }

private:
  void* dalloc(size_t bytes)
  {
    void* p = be_.alloc(bytes);
    if (!p)
      throw EngineError{-5, "correlator: out of memory"};
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
  int quantity_;
  int64_t n_, interval_;
  int num_corr_, num_groups_;
  int64_t ns_ = 0;
  int num_tiles_ = 0, lag_chunk_ = 1, num_chunks_ = 1;
  int64_t num_samples_ = 0, steps_done_ = 0;
  std::vector<void*> allocs_;
  double* ring_ = nullptr;
  double* acc_ = nullptr;
  double* partial_ = nullptr;
  double* weight_ = nullptr;
  int* order_of_ = nullptr;
  CorrTile* tiles_ = nullptr;
  int* tile_first_ = nullptr;
};

} // namespace nepmi
