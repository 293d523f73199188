// vpcc_metrics.hip — point-to-point geometry and colour errors between point clouds (include/vpcc_recon.h, "cloud metrics";
// DESIGN.md §11): vpcc_cloud_errors_compute, vpcc_cloud_nearest, vpcc_gof_cloud_errors.
//
// Every cloud that is a target gets a uniform grid over its bounding box, built by counting sort:
//   k_metrics_bbox      the box, by per-wave min / max and one vector atomic per axis and wave
//   k_metrics_setup     the cell edge: the smallest e whose grid over the box has at most kCellsPerPoint · n cells
//   k_metrics_count     points per cell (vector atomics into the chunk's cell array)
//   k_scan_*            one exclusive scan over the cell arrays of all targets of a chunk, in place: the start of every cell
//                       in the chunk's sorted array (targets lie one after the other in both)
//   k_metrics_scatter   slot = atomicAdd(start[cell], 1): the points sorted by cell — {x | y << 16, z, index}; afterwards
//                       cell[c] is the END of cell c, and the start of cell c is cell[c − 1] (0 for c = 0)
// Then a lane per source point walks its own cell and shells of cells outward (k_metrics_query).  A shell's rows along x are
// contiguous cells, hence ONE contiguous range of sorted points.  The walk stops once the best d² is strictly below the exact
// lower bound of d² to any point outside the visited cube (the nearest face of the cube that has cells beyond it), so a tie
// outside cannot be missed; ties inside are decided by (d², index), which does not depend on the order of the points in a cell
// (which the scatter's atomics decide).  Sums: per lane in a fixed order, per wave by butterfly, per workgroup in wave order
// (k_metrics_query), then per direction over the workgroups' partials in a fixed order (k_metrics_finish): the doubles are
// the same in every run, and the same whichever chunk a pair falls in.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vpcc_runtime.hpp"

using namespace vpcc;

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kQueryPerLane = 4;                          // source points per lane of k_metrics_query
constexpr uint32_t kQueryPerBlock = kThreads * kQueryPerLane;
constexpr uint32_t kScanPerThread = 16;
constexpr uint32_t kScanTile = kThreads * kScanPerThread;       // cells per workgroup of the scan
constexpr uint64_t kCellsPerPoint = 2;                          // grid cells reserved per target point
constexpr uint64_t kMaxCellsPerCloud = uint64_t(1) << 30;
constexpr uint64_t kMaxPerChunk = uint64_t(1) << 31;            // cells, and points, of one chunk (32-bit indices)
constexpr uint64_t kMaxSource = 1431655765ull;                  // 3 · 65535² · n fits 64 bits

struct MetricGrid {                  // one per target cloud
  const vpcc_point3* xyz;
  uint32_t n;
  uint32_t lo[3], hi[3];             // bounding box (host: lo = ~0, hi = 0; k_metrics_bbox)
  uint32_t e;                        // cell edge (k_metrics_setup)
  uint32_t dim[3];
  uint32_t cell_base;                // first cell of the grid in the chunk's cell array
  uint32_t cells;                    // cells reserved (>= dim x · dim y · dim z)
  uint32_t pad;
};
static_assert(sizeof(MetricGrid) == 64, "MetricGrid is 64 B");

struct MetricJob {                   // one per direction source -> target
  const vpcc_point3* sxyz;
  const vpcc_color3* srgb;           // both colour pointers set: colour terms
  const vpcc_color3* trgb;
  uint32_t* idx_out;                 // per-point correspondence (vpcc_cloud_nearest), or null
  uint64_t* d2_out;
  uint32_t n_src, grid;
  uint32_t part_base, blocks;        // the job's workgroup partials: [part_base, part_base + blocks)
};

struct alignas(16) MetricSums {
  uint64_t sse, max;
  uint64_t rgb[3];
  double ycc[3];
};
static_assert(sizeof(MetricSums) == 64, "MetricSums is 64 B");

__device__ inline uint32_t cell_axis(uint32_t p, uint32_t lo, uint32_t e, uint32_t dim) {
  if (p < lo) return 0;
  const uint32_t c = (p - lo) / e;
  return c < dim ? c : dim - 1;
}

// ------------------------------------------------------------------ grid build
__global__ __launch_bounds__(kThreads) void k_metrics_bbox(MetricGrid* __restrict__ grids) {
  MetricGrid& G = grids[blockIdx.y];
  const uint32_t n = G.n;
  uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0, 0, 0};
  for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
    const vpcc_point3 p = G.xyz[i];
    const uint32_t v[3] = {p.x, p.y, p.z};
    for (int a = 0; a < 3; ++a) {
      lo[a] = min(lo[a], v[a]);
      hi[a] = max(hi[a], v[a]);
    }
  }
  for (int off = 32; off > 0; off >>= 1)
    for (int a = 0; a < 3; ++a) {
      lo[a] = min(lo[a], (uint32_t)__shfl_xor((int)lo[a], off, 64));
      hi[a] = max(hi[a], (uint32_t)__shfl_xor((int)hi[a], off, 64));
    }
  if ((threadIdx.x & 63u) == 0 && lo[0] <= hi[0])
    for (int a = 0; a < 3; ++a) {
      atomicMin(&G.lo[a], lo[a]);
      atomicMax(&G.hi[a], hi[a]);
    }
}

__global__ void k_metrics_setup(MetricGrid* __restrict__ grids, uint32_t n_grids) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_grids) return;
  MetricGrid& G = grids[t];
  if (G.n == 0) return;
  uint64_t L[3];
  for (int a = 0; a < 3; ++a) L[a] = (uint64_t)G.hi[a] - G.lo[a] + 1;
  // the cell count falls as e grows: the smallest e in [1, 65536] with at most G.cells cells, by bisection
  uint32_t a = 1, b = 65536;
  while (a < b) {
    const uint32_t m = (a + b) / 2;
    const uint64_t c = ((L[0] + m - 1) / m) * ((L[1] + m - 1) / m) * ((L[2] + m - 1) / m);
    if (c <= G.cells) b = m; else a = m + 1;
  }
  G.e = a;
  for (int k = 0; k < 3; ++k) G.dim[k] = (uint32_t)((L[k] + a - 1) / a);
}

__device__ inline uint32_t grid_cell(const MetricGrid& G, vpcc_point3 p) {
  const uint32_t cx = cell_axis(p.x, G.lo[0], G.e, G.dim[0]);
  const uint32_t cy = cell_axis(p.y, G.lo[1], G.e, G.dim[1]);
  const uint32_t cz = cell_axis(p.z, G.lo[2], G.e, G.dim[2]);
  return G.cell_base + (cz * G.dim[1] + cy) * G.dim[0] + cx;
}

__global__ __launch_bounds__(kThreads) void k_metrics_count(const MetricGrid* __restrict__ grids, uint32_t* __restrict__ cells) {
  const MetricGrid& G = grids[blockIdx.y];
  for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < G.n; i += gridDim.x * kThreads)
    atomicAdd(&cells[grid_cell(G, G.xyz[i])], 1u);
}

__global__ __launch_bounds__(kThreads) void k_metrics_scatter(const MetricGrid* __restrict__ grids, uint32_t* __restrict__ cells,
                                                            uint4* __restrict__ sorted) {
  const MetricGrid& G = grids[blockIdx.y];
  for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < G.n; i += gridDim.x * kThreads) {
    const vpcc_point3 p = G.xyz[i];
    const uint32_t slot = atomicAdd(&cells[grid_cell(G, p)], 1u);
    sorted[slot] = make_uint4((uint32_t)p.x | ((uint32_t)p.y << 16), p.z, i, 0u);
  }
}

// ------------------------------------------------------------------ exclusive scan of the cell counts, in place
// Exclusive scan of v over the block (blockDim.x = 64 · waves <= 1024); *total = the block's sum.
__device__ inline uint32_t block_exclusive_scan(uint32_t v, uint32_t* lds, uint32_t* total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  uint32_t x = v;
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t y = (uint32_t)__shfl_up((int)x, off, 64);
    if (lane >= (uint32_t)off) x += y;
  }
  if (lane == 63) lds[wave] = x;
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (uint32_t w = 0; w < waves; ++w) {
    before += w < wave ? lds[w] : 0u;
    all += lds[w];
  }
  __syncthreads();
  *total = all;
  return before + x - v;
}

__global__ __launch_bounds__(kThreads) void k_scan_tiles(const uint32_t* __restrict__ cells, uint64_t n, uint32_t* __restrict__ sums) {
  __shared__ uint32_t lds[16];
  const uint64_t base = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanPerThread;
  uint32_t s = 0;
  for (uint32_t k = 0; k < kScanPerThread; ++k) s += base + k < n ? cells[base + k] : 0u;
  uint32_t total;
  block_exclusive_scan(s, lds, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// One workgroup of 1 024 lanes: the tiles' sums, scanned in place.
__global__ __launch_bounds__(1024) void k_scan_sums(uint32_t* __restrict__ sums, uint32_t n) {
  __shared__ uint32_t lds[16];
  uint32_t carry = 0;
  for (uint32_t b = 0; b < n; b += 1024) {
    const uint32_t i = b + threadIdx.x;
    const uint32_t v = i < n ? sums[i] : 0u;
    uint32_t total;
    const uint32_t x = block_exclusive_scan(v, lds, &total);
    if (i < n) sums[i] = carry + x;
    carry += total;
  }
}

__global__ __launch_bounds__(kThreads) void k_scan_apply(uint32_t* __restrict__ cells, uint64_t n, const uint32_t* __restrict__ sums) {
  __shared__ uint32_t lds[16];
  const uint64_t base = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanPerThread;
  uint32_t v[kScanPerThread], s = 0;
  for (uint32_t k = 0; k < kScanPerThread; ++k) {
    v[k] = base + k < n ? cells[base + k] : 0u;
    s += v[k];
  }
  uint32_t total;
  uint32_t x = sums[blockIdx.x] + block_exclusive_scan(s, lds, &total);
  for (uint32_t k = 0; k < kScanPerThread; ++k) {
    if (base + k < n) cells[base + k] = x;
    x += v[k];
  }
}

// ------------------------------------------------------------------ the search
// Sorted points [b, e) against p: the best (d², index) so far, lexicographically.
__device__ inline void scan_range(const uint4* __restrict__ sorted, uint32_t b, uint32_t e, uint32_t px, uint32_t py, uint32_t pz,
                                  uint64_t& best, uint32_t& bi) {
  for (uint32_t k = b; k < e; ++k) {
    const uint4 q = sorted[k];
    const uint32_t qx = q.x & 0xFFFFu, qy = q.x >> 16, qz = q.y;
    const uint32_t dx = qx > px ? qx - px : px - qx, dy = qy > py ? qy - py : py - qy, dz = qz > pz ? qz - pz : pz - qz;
    const uint64_t d2 = (uint64_t)(dx * dx) + (uint64_t)(dy * dy) + (uint64_t)(dz * dz);   // (each square < 2^32)
    if (d2 < best || (d2 == best && q.z < bi)) {
      best = d2;
      bi = q.z;
    }
  }
}

__device__ inline uint32_t cell_begin(const uint32_t* __restrict__ cells, uint32_t c) { return c ? cells[c - 1] : 0u; }

// The nearest neighbour of p in G: (d², index).
__device__ inline void nearest(const MetricGrid& G, const uint32_t* __restrict__ cells, const uint4* __restrict__ sorted,
                               vpcc_point3 p, uint64_t& best, uint32_t& bi) {
  const int dx = (int)G.dim[0], dy = (int)G.dim[1], dz = (int)G.dim[2];
  const int cx = (int)cell_axis(p.x, G.lo[0], G.e, G.dim[0]);
  const int cy = (int)cell_axis(p.y, G.lo[1], G.e, G.dim[1]);
  const int cz = (int)cell_axis(p.z, G.lo[2], G.e, G.dim[2]);
  const int c[3] = {cx, cy, cz}, d[3] = {dx, dy, dz};
  const int64_t pv[3] = {p.x, p.y, p.z};
  best = ~0ull;
  bi = ~0u;
  for (int r = 0;; ++r) {
    const int x0 = max(cx - r, 0), x1 = min(cx + r, dx - 1);
    const int y0 = max(cy - r, 0), y1 = min(cy + r, dy - 1);
    const int z0 = max(cz - r, 0), z1 = min(cz + r, dz - 1);
    for (int z = z0; z <= z1; ++z) {
      const bool zs = z == cz - r || z == cz + r;
      for (int y = y0; y <= y1; ++y) {
        const uint32_t row = G.cell_base + ((uint32_t)z * G.dim[1] + (uint32_t)y) * G.dim[0];
        if (zs || y == cy - r || y == cy + r) {            // a face of the shell: the whole row, one range
          scan_range(sorted, cell_begin(cells, row + x0), cells[row + x1], p.x, p.y, p.z, best, bi);
        } else {                                           // inside: the shell's two cells of the row
          if (cx - r >= 0) scan_range(sorted, cell_begin(cells, row + cx - r), cells[row + cx - r], p.x, p.y, p.z, best, bi);
          if (cx + r < dx) scan_range(sorted, cell_begin(cells, row + cx + r), cells[row + cx + r], p.x, p.y, p.z, best, bi);
        }
      }
    }
    // Every point outside the visited cube lies beyond one of its faces that has cells behind it: d² >= (distance to that
    // face's first coordinate outside)².
    uint64_t lb = ~0ull;
    for (int a = 0; a < 3; ++a) {
      if (c[a] - r > 0) {
        const int64_t t = pv[a] - ((int64_t)G.lo[a] + (int64_t)(c[a] - r) * G.e - 1);
        const uint64_t u = t > 0 ? (uint64_t)t : 0;
        lb = min(lb, u * u);
      }
      if (c[a] + r < d[a] - 1) {
        const int64_t t = ((int64_t)G.lo[a] + (int64_t)(c[a] + r + 1) * G.e) - pv[a];
        const uint64_t u = t > 0 ? (uint64_t)t : 0;
        lb = min(lb, u * u);
      }
    }
    if (lb == ~0ull || best < lb) return;                  // the whole grid visited, or nothing outside can tie or win
  }
}

template <typename T>
__device__ inline T wave_sum(T v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ __launch_bounds__(kThreads) void k_metrics_query(const MetricJob* __restrict__ jobs, const MetricGrid* __restrict__ grids,
                                                          const uint32_t* __restrict__ cells, const uint4* __restrict__ sorted,
                                                          MetricSums* __restrict__ partials) {
  const MetricJob& J = jobs[blockIdx.y];
  if (blockIdx.x >= J.blocks) return;
  const MetricGrid& G = grids[J.grid];
  const bool colour = J.srgb && J.trgb && G.n;
  unsigned long long sse = 0, mx = 0, rgb[3] = {0, 0, 0};
  double ycc[3] = {0, 0, 0};
  for (uint32_t k = 0; k < kQueryPerLane; ++k) {
    const uint32_t i = blockIdx.x * kQueryPerBlock + k * kThreads + threadIdx.x;
    if (i >= J.n_src) break;
    uint64_t best = ~0ull;
    uint32_t bi = ~0u;
    if (G.n) {
      nearest(G, cells, sorted, J.sxyz[i], best, bi);
      sse += best;
      mx = max(mx, (unsigned long long)best);
      if (colour) {
        const vpcc_color3 a = J.srgb[i], b = J.trgb[bi];
        const int dr = (int)a.r - (int)b.r, dg = (int)a.g - (int)b.g, db = (int)a.b - (int)b.b;
        rgb[0] += (unsigned long long)(dr * dr);
        rgb[1] += (unsigned long long)(dg * dg);
        rgb[2] += (unsigned long long)(db * db);
        const double R = dr, Gd = dg, B = db;
        const double y = 0.2126 * R + 0.7152 * Gd + 0.0722 * B;         // left to right, no contraction (-ffp-contract=off)
        const double cb = -0.1146 * R - 0.3854 * Gd + 0.5 * B;
        const double cr = 0.5 * R - 0.4542 * Gd - 0.0458 * B;
        ycc[0] += y * y;
        ycc[1] += cb * cb;
        ycc[2] += cr * cr;
      }
    }
    if (J.idx_out) J.idx_out[i] = bi;
    if (J.d2_out) J.d2_out[i] = best;
  }
  __shared__ MetricSums wsum[kThreads / 64];
  sse = wave_sum(sse);
  for (int off = 32; off > 0; off >>= 1) mx = max(mx, (unsigned long long)__shfl_xor(mx, off, 64));
  for (int c = 0; c < 3; ++c) {
    rgb[c] = wave_sum(rgb[c]);
    ycc[c] = wave_sum(ycc[c]);
  }
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) {
    wsum[wave].sse = sse;
    wsum[wave].max = mx;
    for (int c = 0; c < 3; ++c) {
      wsum[wave].rgb[c] = rgb[c];
      wsum[wave].ycc[c] = ycc[c];
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    MetricSums s = wsum[0];
    for (uint32_t w = 1; w < kThreads / 64; ++w) {
      s.sse += wsum[w].sse;
      s.max = max(s.max, wsum[w].max);
      for (int c = 0; c < 3; ++c) {
        s.rgb[c] += wsum[w].rgb[c];
        s.ycc[c] += wsum[w].ycc[c];
      }
    }
    partials[J.part_base + blockIdx.x] = s;
  }
}

// One wave per job: its partials in a fixed order (lane l: l, l + 64, ...; then a butterfly).
__global__ __launch_bounds__(64) void k_metrics_finish(const MetricJob* __restrict__ jobs, const MetricSums* __restrict__ partials,
                                                      MetricSums* __restrict__ out) {
  const MetricJob& J = jobs[blockIdx.x];
  unsigned long long sse = 0, mx = 0, rgb[3] = {0, 0, 0};
  double ycc[3] = {0, 0, 0};
  for (uint32_t b = threadIdx.x; b < J.blocks; b += 64) {
    const MetricSums& s = partials[J.part_base + b];
    sse += s.sse;
    mx = max(mx, (unsigned long long)s.max);
    for (int c = 0; c < 3; ++c) {
      rgb[c] += s.rgb[c];
      ycc[c] += s.ycc[c];
    }
  }
  sse = wave_sum(sse);
  for (int off = 32; off > 0; off >>= 1) mx = max(mx, (unsigned long long)__shfl_xor(mx, off, 64));
  for (int c = 0; c < 3; ++c) {
    rgb[c] = wave_sum(rgb[c]);
    ycc[c] = wave_sum(ycc[c]);
  }
  if (threadIdx.x == 0) {
    MetricSums s;
    s.sse = sse;
    s.max = mx;
    for (int c = 0; c < 3; ++c) {
      s.rgb[c] = rgb[c];
      s.ycc[c] = ycc[c];
    }
    out[blockIdx.x] = s;
  }
}

// ------------------------------------------------------------------ host side
struct CloudIn {
  vpcc_cloud c;
  bool host;                         // VPCC_MEM_HOST: staged into the scratch
  bool target;                       // a grid is built over it
};
struct JobIn {
  uint32_t src, tgt;                 // indices into the chunk's clouds
  uint32_t* idx_out;                 // outputs of vpcc_cloud_nearest (host or device, as `out_host` says), or null
  uint64_t* d2_out;
  bool out_host;
};

uint64_t cloud_cells(const vpcc_cloud& c) { return c.n ? std::min<uint64_t>(kCellsPerPoint * c.n, kMaxCellsPerCloud) : 0; }
uint32_t job_blocks(uint32_t n_src) { return (n_src + kQueryPerBlock - 1) / kQueryPerBlock; }

// Scratch of a chunk, at most: what the chunker adds up and run_chunk lays out.
uint64_t cloud_bytes(const CloudIn& c) {
  uint64_t b = 0;
  if (c.target) b += 4 * cloud_cells(c.c) + 4 * (cloud_cells(c.c) / kScanTile + 1) + 16ull * c.c.n + sizeof(MetricGrid) + 1024;
  if (c.host) b += 6ull * c.c.n + 3ull * c.c.n + 512;
  return b;
}
uint64_t job_bytes(const JobIn& j, uint32_t n_src) {
  uint64_t b = sizeof(MetricSums) * (job_blocks(n_src) + 1) + sizeof(MetricJob) + 512;
  if (j.out_host && (j.idx_out || j.d2_out)) b += 12ull * n_src + 512;
  return b;
}

int ensure_scratch(vpcc_ctx* ctx, size_t bytes, size_t host_bytes) {
  if (ctx->metrics_bytes < bytes) {
    if (ctx->metrics_scratch) HIP_TRY(ctx, hipFree(ctx->metrics_scratch));
    ctx->metrics_scratch = nullptr;
    ctx->metrics_bytes = 0;
    HIP_TRY(ctx, device_malloc(ctx, &ctx->metrics_scratch, bytes));
    ctx->metrics_bytes = bytes;
  }
  if (ctx->metrics_host_bytes < host_bytes) {
    if (ctx->metrics_host) HIP_TRY(ctx, hipHostFree(ctx->metrics_host));
    ctx->metrics_host = nullptr;
    ctx->metrics_host_bytes = 0;
    HIP_TRY(ctx, hipHostMalloc(&ctx->metrics_host, host_bytes, hipHostMallocDefault));
    ctx->metrics_host_bytes = host_bytes;
  }
  return VPCC_OK;
}

// One chunk: grids over its target clouds, every job, its sums into out[n_jobs].  Waits for the result.
// Every copy between host and device goes through the context's page-locked staging buffer: the caller's (pageable) memory is
// touched by the CPU only, never handed to the HIP runtime's copy paths.
int run_chunk(vpcc_ctx* ctx, hipStream_t s, const std::vector<CloudIn>& clouds, const std::vector<JobIn>& jobs, MetricSums* out) {
  // layout: `at` on the device, `hat` in the page-locked staging buffer
  size_t at = 0, hat = 0;
  auto take = [&](size_t bytes) { const size_t o = at; at = align_up(at + bytes, 256); return o; };
  auto htake = [&](size_t bytes) { const size_t o = hat; hat = align_up(hat + bytes, 256); return o; };
  std::vector<size_t> xyz_off(clouds.size(), 0), rgb_off(clouds.size(), 0);
  std::vector<size_t> hxyz_off(clouds.size(), 0), hrgb_off(clouds.size(), 0);
  std::vector<uint32_t> grid_of(clouds.size(), ~0u);
  std::vector<MetricGrid> grids;
  uint64_t cells = 0, points = 0;
  uint32_t max_target = 0;
  for (size_t k = 0; k < clouds.size(); ++k) {
    const CloudIn& C = clouds[k];
    if (C.host) {
      xyz_off[k] = take(6ull * C.c.n);
      rgb_off[k] = C.c.rgb ? take(3ull * C.c.n) : 0;
      hxyz_off[k] = htake(6ull * C.c.n);
      hrgb_off[k] = C.c.rgb ? htake(3ull * C.c.n) : 0;
    }
    if (!C.target) continue;
    MetricGrid G{};
    G.n = C.c.n;
    for (int a = 0; a < 3; ++a) { G.lo[a] = 0xFFFFFFFFu; G.hi[a] = 0; }
    G.cell_base = (uint32_t)cells;
    G.cells = (uint32_t)cloud_cells(C.c);
    cells += G.cells;
    points += C.c.n;
    max_target = std::max(max_target, C.c.n);
    grid_of[k] = (uint32_t)grids.size();
    grids.push_back(G);
  }
  if (cells > kMaxPerChunk || points > kMaxPerChunk) return fail(ctx, VPCC_ERR_UNSUPPORTED, "cloud metrics: chunk beyond 2^31 cells or points");
  const uint64_t tiles = (cells + kScanTile - 1) / kScanTile;
  const size_t grids_off = take(sizeof(MetricGrid) * std::max<size_t>(grids.size(), 1));
  const size_t cells_off = take(4 * std::max<uint64_t>(cells, 1));
  const size_t tiles_off = take(4 * std::max<uint64_t>(tiles, 1));
  const size_t sorted_off = take(16 * std::max<uint64_t>(points, 1));
  std::vector<MetricJob> dj(jobs.size());
  uint64_t parts = 0;
  uint32_t max_blocks = 0;
  std::vector<size_t> out_off(jobs.size(), 0), hout_off(jobs.size(), 0);
  for (size_t j = 0; j < jobs.size(); ++j) {
    const JobIn& J = jobs[j];
    MetricJob& D = dj[j];
    D.n_src = clouds[J.src].c.n;
    D.grid = grid_of[J.tgt];
    D.blocks = job_blocks(D.n_src);
    D.part_base = (uint32_t)parts;
    parts += D.blocks;
    max_blocks = std::max(max_blocks, D.blocks);
    if (J.out_host && (J.idx_out || J.d2_out)) {
      out_off[j] = take(12ull * D.n_src + 8);
      hout_off[j] = htake(12ull * D.n_src + 8);
    }
  }
  const size_t jobs_off = take(sizeof(MetricJob) * std::max<size_t>(jobs.size(), 1));
  const size_t parts_off = take(sizeof(MetricSums) * (parts + jobs.size() + 1));
  const size_t hgrids_off = htake(sizeof(MetricGrid) * std::max<size_t>(grids.size(), 1));
  const size_t hjobs_off = htake(sizeof(MetricJob) * std::max<size_t>(jobs.size(), 1));
  const size_t hres_off = htake(sizeof(MetricSums) * std::max<size_t>(jobs.size(), 1));
  int st = ensure_scratch(ctx, at, hat);
  if (st) return st;
  char* base = (char*)ctx->metrics_scratch;
  char* hbase = (char*)ctx->metrics_host;
  // stage host clouds, point grids and jobs at the device copies
  for (size_t k = 0; k < clouds.size(); ++k) {
    const CloudIn& C = clouds[k];
    const vpcc_point3* xyz = C.c.xyz;
    const vpcc_color3* rgb = C.c.rgb;
    if (C.host) {
      if (C.c.n) {
        std::memcpy(hbase + hxyz_off[k], C.c.xyz, 6ull * C.c.n);
        HIP_TRY(ctx, hipMemcpyAsync(base + xyz_off[k], hbase + hxyz_off[k], 6ull * C.c.n, hipMemcpyHostToDevice, s));
      }
      if (C.c.n && rgb) {
        std::memcpy(hbase + hrgb_off[k], C.c.rgb, 3ull * C.c.n);
        HIP_TRY(ctx, hipMemcpyAsync(base + rgb_off[k], hbase + hrgb_off[k], 3ull * C.c.n, hipMemcpyHostToDevice, s));
      }
      xyz = (const vpcc_point3*)(base + xyz_off[k]);
      rgb = rgb ? (const vpcc_color3*)(base + rgb_off[k]) : nullptr;
    }
    if (grid_of[k] != ~0u) grids[grid_of[k]].xyz = xyz;
    for (size_t j = 0; j < jobs.size(); ++j) {
      if (jobs[j].src == k) { dj[j].sxyz = xyz; dj[j].srgb = rgb; }
      if (jobs[j].tgt == k) dj[j].trgb = rgb;
    }
  }
  for (size_t j = 0; j < jobs.size(); ++j) {
    const JobIn& J = jobs[j];
    if (!dj[j].srgb || !dj[j].trgb) dj[j].srgb = dj[j].trgb = nullptr;
    if (J.out_host && (J.idx_out || J.d2_out)) {
      dj[j].d2_out = (uint64_t*)(base + out_off[j]);
      dj[j].idx_out = (uint32_t*)(base + out_off[j] + 8ull * dj[j].n_src);
    } else {
      dj[j].idx_out = J.idx_out;
      dj[j].d2_out = J.d2_out;
    }
  }
  MetricGrid* d_grids = (MetricGrid*)(base + grids_off);
  uint32_t* d_cells = (uint32_t*)(base + cells_off);
  uint32_t* d_tiles = (uint32_t*)(base + tiles_off);
  uint4* d_sorted = (uint4*)(base + sorted_off);
  MetricJob* d_jobs = (MetricJob*)(base + jobs_off);
  MetricSums* d_parts = (MetricSums*)(base + parts_off);
  MetricSums* d_out = d_parts + parts;
  if (!grids.empty()) {
    std::memcpy(hbase + hgrids_off, grids.data(), sizeof(MetricGrid) * grids.size());
    HIP_TRY(ctx, hipMemcpyAsync(d_grids, hbase + hgrids_off, sizeof(MetricGrid) * grids.size(), hipMemcpyHostToDevice, s));
  }
  if (!jobs.empty()) {
    std::memcpy(hbase + hjobs_off, dj.data(), sizeof(MetricJob) * dj.size());
    HIP_TRY(ctx, hipMemcpyAsync(d_jobs, hbase + hjobs_off, sizeof(MetricJob) * dj.size(), hipMemcpyHostToDevice, s));
  }
  // grids
  if (!grids.empty() && points) {
    const uint32_t ng = (uint32_t)grids.size();
    const uint32_t bx = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((max_target + 2047) / 2048, std::max<uint32_t>(1, 65536 / ng)));
    const dim3 grid(bx, ng);
    HIP_TRY(ctx, hipMemsetAsync(d_cells, 0, 4 * cells, s));
    hipLaunchKernelGGL(k_metrics_bbox, grid, dim3(kThreads), 0, s, d_grids);
    hipLaunchKernelGGL(k_metrics_setup, dim3((ng + 63) / 64), dim3(64), 0, s, d_grids, ng);
    hipLaunchKernelGGL(k_metrics_count, grid, dim3(kThreads), 0, s, d_grids, d_cells);
    hipLaunchKernelGGL(k_scan_tiles, dim3((uint32_t)tiles), dim3(kThreads), 0, s, d_cells, cells, d_tiles);
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(1024), 0, s, d_tiles, (uint32_t)tiles);
    hipLaunchKernelGGL(k_scan_apply, dim3((uint32_t)tiles), dim3(kThreads), 0, s, d_cells, cells, d_tiles);
    hipLaunchKernelGGL(k_metrics_scatter, grid, dim3(kThreads), 0, s, d_grids, d_cells, d_sorted);
  }
  if (!jobs.empty()) {
    if (max_blocks) hipLaunchKernelGGL(k_metrics_query, dim3(max_blocks, (uint32_t)jobs.size()), dim3(kThreads), 0, s, d_jobs, d_grids,
                                       d_cells, d_sorted, d_parts);
    hipLaunchKernelGGL(k_metrics_finish, dim3((uint32_t)jobs.size()), dim3(64), 0, s, d_jobs, d_parts, d_out);
  }
  HIP_TRY(ctx, hipGetLastError());
  for (size_t j = 0; j < jobs.size(); ++j) {
    const JobIn& J = jobs[j];
    const uint64_t n = dj[j].n_src;
    if (!J.out_host || !n || !(J.idx_out || J.d2_out)) continue;
    // (the device copy of the outputs is d2 then index, 12n + 8 bytes: mirrored as one piece)
    HIP_TRY(ctx, hipMemcpyAsync(hbase + hout_off[j], base + out_off[j], 12 * n + 8, hipMemcpyDeviceToHost, s));
  }
  if (!jobs.empty()) HIP_TRY(ctx, hipMemcpyAsync(hbase + hres_off, d_out, sizeof(MetricSums) * jobs.size(), hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  for (size_t j = 0; j < jobs.size(); ++j) {
    const JobIn& J = jobs[j];
    const uint64_t n = dj[j].n_src;
    if (!J.out_host || !n || !(J.idx_out || J.d2_out)) continue;
    if (J.d2_out) std::memcpy(J.d2_out, hbase + hout_off[j], 8 * n);
    if (J.idx_out) std::memcpy(J.idx_out, hbase + hout_off[j] + 8 * n, 4 * n);
  }
  if (!jobs.empty()) std::memcpy(out, hbase + hres_off, sizeof(MetricSums) * jobs.size());
  return VPCC_OK;
}

int check_cloud(vpcc_ctx* ctx, const vpcc_cloud& c) {
  if (c.n && !c.xyz) return fail(ctx, VPCC_ERR_INVALID_ARG, "cloud of n > 0 points without positions");
  return VPCC_OK;
}

void fill_errors(const MetricSums& s, const vpcc_cloud& src, const vpcc_cloud& tgt, vpcc_cloud_errors* e) {
  std::memset(e, 0, sizeof *e);
  e->n_src = src.n;
  e->n_tgt = tgt.n;
  e->has_color = src.rgb && tgt.rgb ? 1u : 0u;
  e->geo_sse = s.sse;
  e->geo_max = s.max;
  if (!e->has_color) return;
  for (int c = 0; c < 3; ++c) {
    e->rgb_sse[c] = s.rgb[c];
    e->ycc_sse[c] = s.ycc[c];
  }
}

// Both directions of every pair (a[i], b[i]), in chunks whose scratch fits the limit.
int pair_errors(vpcc_ctx* ctx, hipStream_t s, const vpcc_cloud* a, bool a_host, const vpcc_cloud* b, bool b_host, uint32_t n_pairs,
                vpcc_cloud_errors* ab_out, vpcc_cloud_errors* ba_out) {
  for (uint32_t i = 0; i < n_pairs; ++i) {
    int st = check_cloud(ctx, a[i]);
    if (!st) st = check_cloud(ctx, b[i]);
    if (st) return st;
    if (a[i].n > kMaxSource || b[i].n > kMaxSource)
      return fail(ctx, VPCC_ERR_UNSUPPORTED, "cloud metrics: a source of more than 1 431 655 765 points (geo_sse could overflow)");
    if ((uint64_t)a[i].n + b[i].n > kMaxPerChunk) return fail(ctx, VPCC_ERR_UNSUPPORTED, "cloud metrics: a pair of more than 2^31 points");
  }
  // (VPCC_METRICS_SCRATCH_LIMIT_MB: the limit in MB, for tests that want several chunks out of a few pairs)
  const char* limit_env = getenv("VPCC_METRICS_SCRATCH_LIMIT_MB");
  const uint64_t limit = limit_env ? std::max<uint64_t>(1, (uint64_t)atoll(limit_env)) << 20 : uint64_t(4) << 30;
  std::vector<MetricSums> sums;
  for (uint32_t i0 = 0; i0 < n_pairs;) {
    std::vector<CloudIn> clouds;
    std::vector<JobIn> jobs;
    uint64_t bytes = 4096, cells = 0, points = 0;
    uint32_t i = i0;
    for (; i < n_pairs; ++i) {
      const CloudIn A{a[i], a_host, true}, B{b[i], b_host, true};
      const JobIn ab{(uint32_t)clouds.size(), (uint32_t)clouds.size() + 1, nullptr, nullptr, false};
      const JobIn ba{(uint32_t)clouds.size() + 1, (uint32_t)clouds.size(), nullptr, nullptr, false};
      const uint64_t add = cloud_bytes(A) + cloud_bytes(B) + job_bytes(ab, a[i].n) + job_bytes(ba, b[i].n);
      const uint64_t add_cells = cloud_cells(a[i]) + cloud_cells(b[i]), add_points = (uint64_t)a[i].n + b[i].n;
      if (i > i0 && (bytes + add > limit || cells + add_cells > kMaxPerChunk || points + add_points > kMaxPerChunk ||
                     jobs.size() + 2 > 65535))
        break;
      bytes += add;
      cells += add_cells;
      points += add_points;
      clouds.push_back(A);
      clouds.push_back(B);
      jobs.push_back(ab);
      jobs.push_back(ba);
    }
    sums.assign(jobs.size(), MetricSums{});
    const int st = run_chunk(ctx, s, clouds, jobs, sums.data());
    if (st) return st;
    for (uint32_t k = i0; k < i; ++k) {
      fill_errors(sums[2 * (k - i0)], a[k], b[k], &ab_out[k]);
      fill_errors(sums[2 * (k - i0) + 1], b[k], a[k], &ba_out[k]);
    }
    i0 = i;
  }
  return VPCC_OK;
}

}  // namespace

extern "C" int vpcc_cloud_errors_compute(vpcc_ctx* ctx, const vpcc_cloud* a, const vpcc_cloud* b, uint32_t n_pairs,
                                         vpcc_memory_kind mem, vpcc_cloud_errors* ab_out, vpcc_cloud_errors* ba_out) {
  if (!ctx || (n_pairs && (!a || !b || !ab_out || !ba_out))) return VPCC_ERR_INVALID_ARG;
  if (mem != VPCC_MEM_HOST && mem != VPCC_MEM_DEVICE) return fail(ctx, VPCC_ERR_INVALID_ARG, "memory kind");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return pair_errors(ctx, ctx->stream, a, mem == VPCC_MEM_HOST, b, mem == VPCC_MEM_HOST, n_pairs, ab_out, ba_out);
}

extern "C" int vpcc_cloud_nearest(vpcc_ctx* ctx, const vpcc_cloud* s, const vpcc_cloud* t, vpcc_memory_kind mem, uint32_t* index_out,
                                  uint64_t* dist2_out) {
  if (!ctx || !s || !t) return VPCC_ERR_INVALID_ARG;
  if (mem != VPCC_MEM_HOST && mem != VPCC_MEM_DEVICE) return fail(ctx, VPCC_ERR_INVALID_ARG, "memory kind");
  int st = check_cloud(ctx, *s);
  if (!st) st = check_cloud(ctx, *t);
  if (st) return st;
  if (s->n > kMaxSource) return fail(ctx, VPCC_ERR_UNSUPPORTED, "cloud metrics: a source of more than 1 431 655 765 points");
  if ((uint64_t)s->n + t->n > kMaxPerChunk) return fail(ctx, VPCC_ERR_UNSUPPORTED, "cloud metrics: a pair of more than 2^31 points");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const bool host = mem == VPCC_MEM_HOST;
  vpcc_cloud src = *s;
  src.rgb = nullptr;                                       // (the correspondence needs no colours)
  const std::vector<CloudIn> clouds{{src, host, false}, {*t, host, true}};
  const std::vector<JobIn> jobs{{0, 1, index_out, dist2_out, host}};
  MetricSums sums{};
  return run_chunk(ctx, ctx->stream, clouds, jobs, &sums);
}

extern "C" int vpcc_gof_cloud_errors(vpcc_gof* g, uint32_t first, uint32_t count, const vpcc_cloud* refs, vpcc_memory_kind mem,
                                     vpcc_cloud_errors* ab_out, vpcc_cloud_errors* ba_out) {
  if (!g || !refs || !ab_out || !ba_out) return VPCC_ERR_INVALID_ARG;
  vpcc_ctx* ctx = g->ctx;
  if (count == 0 || first >= g->n_frames || count > g->n_frames - first) return fail(ctx, VPCC_ERR_INVALID_ARG, "frame range");
  if (mem != VPCC_MEM_HOST && mem != VPCC_MEM_DEVICE) return fail(ctx, VPCC_ERR_INVALID_ARG, "memory kind");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!g->launched) return fail(ctx, VPCC_ERR_STATE, "no reconstruct issued");
  // the point counts as the gof's latest launch left them (waits for it)
  std::vector<uint32_t> counts(g->n_frames);
  int st = vpcc_gof_point_counts(g, counts.data());
  if (st) return st;
  std::vector<vpcc_cloud> a(count);
  for (uint32_t k = 0; k < count; ++k) {
    const DevFrame& D = g->h_frames[first + k];
    if (counts[first + k] > g->capacity)
      return fail(ctx, VPCC_ERR_CAPACITY, "frame " + std::to_string(first + k) + ": its last launch overflowed the capacity");
    a[k] = vpcc_cloud{D.out_xyz, D.has_attr ? D.out_rgb : nullptr, counts[first + k], 0u};
  }
  hipStream_t s = g->last_stream ? g->last_stream : ctx->stream;
  HIP_TRY(ctx, hipStreamWaitEvent(s, g->results_ready, 0));
  st = pair_errors(ctx, s, a.data(), false, refs, mem == VPCC_MEM_HOST, count, ab_out, ba_out);
  if (st) return st;
  HIP_TRY(ctx, hipEventRecord(g->results_ready, s));       // (the gof's next launch is ordered behind the reads)
  return VPCC_OK;
}
