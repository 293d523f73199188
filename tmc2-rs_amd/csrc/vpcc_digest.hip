// vpcc_digest.hip — frame digests on the device (include/vpcc_recon.h, "frame digests"): k_digest_outputs over the frames'
// reconstructed points, k_digest_planes over their device planes, and the gof calls around them.
//
// Both kernels are reductions of a sum of independent 64-bit terms, one per 8-byte word: a lane takes 16 bytes at a time (two
// words) where the row allows it, sums its terms, the wave adds its 64 lanes' partial sums by butterfly (__shfl_xor on 64-bit
// values — the Makefile turns the compiler's atomic optimizer off, so this is done by hand) and issues ONE 64-bit atomicAdd into
// the frame's slot, which was zeroed in stream order in front of the kernel.  The sum commutes: the order in which waves land
// cannot change the result.
#include <algorithm>
#include <cstring>

#include "vpcc_digest.hpp"
#include "vpcc_runtime.hpp"

using namespace vpcc;

namespace {

constexpr uint32_t kDigestThreads = 256;
constexpr uint32_t kDigestTargetBlocks = 4096;   // over all frames of a launch: 16 per CU

// Word k of a row of `bytes` bytes, zero-padded at its end.  8-byte aligned rows: one load (an aligned word never crosses a
// page, so the bytes behind the row's end that it reads are masked, never faulted on); others byte by byte.
__device__ inline uint64_t row_word(const unsigned char* row, uint64_t bytes, uint64_t k) {
  const uint64_t at = 8 * k, left = bytes - at;
  if (((uintptr_t)row & 7u) == 0) {
    uint64_t q = *(const uint64_t*)(row + at);
    if (left < 8) q &= (1ull << (8 * left)) - 1ull;
    return q;
  }
  uint64_t q = 0;
  const uint32_t nb = left < 8 ? (uint32_t)left : 8u;
  for (uint32_t b = 0; b < nb; ++b) q |= (uint64_t)row[at + b] << (8 * b);
  return q;
}

// Σ over the words of word pair j (words 2j, 2j+1) of row (p, y): 16 bytes in one load where the row is 16-byte aligned and
// holds both words whole.
__device__ inline uint64_t row_pair(const unsigned char* row, uint64_t bytes, uint64_t p, uint64_t y, uint64_t j) {
  const uint64_t k = 2 * j;
  if (((uintptr_t)row & 15u) == 0 && 16 * j + 16 <= bytes) {
    typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
    const u64x2 q = *(const u64x2*)(row + 16 * j);
    return digest_term(q.x, p, y, k) + digest_term(q.y, p, y, k + 1);
  }
  uint64_t s = digest_term(row_word(row, bytes, k), p, y, k);
  if (8 * (k + 1) < bytes) s += digest_term(row_word(row, bytes, k + 1), p, y, k + 1);
  return s;
}

__device__ inline void wave_add(uint64_t v, unsigned long long* slot) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor((unsigned long long)v, off, 64);
  if ((threadIdx.x & 63u) == 0) atomicAdd(slot, (unsigned long long)v);
}

// One frame per blockIdx.y.  Its rows, in order: occupancy (occ_h), then per map geometry (H), and with attributes Y (H),
// U (H/2), V (H/2) — or, interleaved chroma (VPCC_FRAME_UV_INTERLEAVED), the U,V rows (H/2) of attr_u as one row set p = 4 + 3m.
// A wave takes one row at a time, its lanes the row's word pairs.
__global__ __launch_bounds__(kDigestThreads) void k_digest_planes(const DevFrame* __restrict__ frames, uint32_t first,
                                                                unsigned long long* __restrict__ slots) {
  const uint32_t f = first + blockIdx.y;
  const DevFrame& D = frames[f];
  const uint64_t W = D.width, H = D.height;
  const bool uv = layout_uv(D.layout);
  const uint64_t per_map = H + (D.has_attr ? H + (uv ? 1 : 2) * (H / 2) : 0);
  const uint64_t rows = D.occ_h + D.map_count * per_map;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = (uint64_t)gridDim.x * (kDigestThreads / 64);
  uint64_t s = (blockIdx.x == 0 && threadIdx.x == 0) ? digest_head((W << 32) | H) : 0;
  for (uint64_t r = (uint64_t)blockIdx.x * (kDigestThreads / 64) + (threadIdx.x >> 6); r < rows; r += waves) {
    const unsigned char* row;
    uint64_t bytes, p, y;
    if (r < D.occ_h) {
      p = 0; y = r; bytes = D.occ_w;
      row = D.occ + y * D.occ_stride;
    } else {
      const uint64_t q = r - D.occ_h, m = q / per_map;
      uint64_t t = q % per_map;
      if (t < H) {
        p = 1 + m; y = t; bytes = 2 * W;
        row = (const unsigned char*)(D.geo[m] + y * D.geo_stride[m]);
      } else if ((t -= H) < H) {
        p = 3 + 3 * m; y = t; bytes = 2 * W;
        row = (const unsigned char*)(D.attr_y[m] + y * D.attr_stride[m]);
      } else {
        t -= H;
        const uint64_t c = t / (H / 2);
        p = 4 + 3 * m + c; y = t % (H / 2); bytes = (uv ? 4 : 2) * (W / 2);       // (interleaved: c == 0 only)
        row = (const unsigned char*)((c ? D.attr_v[m] : D.attr_u[m]) + y * D.attr_cstride[m]);
      }
    }
    const uint64_t pairs = (bytes + 15) / 16;
    for (uint64_t j = lane; j < pairs; j += 64) s += row_pair(row, bytes, p, y, j);
  }
  wave_add(s, slots + f);
}

// One frame per blockIdx.y: head = its device point count n, rows (0, 0, 6n bytes of positions) and (1, 0, 3n bytes of colours).
// Rows are cut at the frame's capacity (a launch that overflowed it wrote no further).
__global__ __launch_bounds__(kDigestThreads) void k_digest_outputs(const DevFrame* __restrict__ frames, uint32_t first,
                                                                 unsigned long long* __restrict__ slots) {
  const uint32_t f = first + blockIdx.y;
  const DevFrame& D = frames[f];
  const uint64_t count = *D.n_points;
  const uint64_t n = count < D.capacity ? count : D.capacity;
  const uint64_t bx = 6 * n, bc = D.out_rgb ? 3 * n : 0;
  const uint64_t px = (bx + 15) / 16, pc = (bc + 15) / 16;
  const unsigned char* xyz = (const unsigned char*)D.out_xyz;
  const unsigned char* rgb = (const unsigned char*)D.out_rgb;
  uint64_t s = (blockIdx.x == 0 && threadIdx.x == 0) ? digest_head(count) : 0;
  for (uint64_t i = (uint64_t)blockIdx.x * kDigestThreads + threadIdx.x; i < px + pc; i += (uint64_t)gridDim.x * kDigestThreads)
    s += i < px ? row_pair(xyz, bx, 0, 0, i) : row_pair(rgb, bc, 1, 0, i - px);
  wave_add(s, slots + f);
}

__global__ void k_flip_byte(unsigned char* p) { *p ^= 1u; }

uint32_t blocks_per_frame(uint32_t count, uint64_t work_bound, uint64_t per_block) {
  const uint64_t want = (kDigestTargetBlocks + count - 1) / count;
  const uint64_t need = std::max<uint64_t>(1, (work_bound + per_block - 1) / per_block);
  return (uint32_t)std::min<uint64_t>(std::min(want, need), 65535);
}

int ensure_digest_buffers(vpcc_gof* g) {
  if (g->digest.bufs.dev) return VPCC_OK;
  vpcc_ctx* ctx = g->ctx;
  const size_t bytes = sizeof(uint64_t) * kDigestSlots * g->n_frames;
  for (size_t k = 0; k < ctx->digest_cache.size(); ++k)
    if (ctx->digest_cache[k].bytes >= bytes) {
      g->digest.bufs = ctx->digest_cache[k];
      ctx->digest_cache.erase(ctx->digest_cache.begin() + (long)k);
      break;
    }
  if (!g->digest.bufs.dev) {
    vpcc_ctx::DigestBuffers b{nullptr, nullptr, std::max<size_t>(bytes, 4096)};
    if (device_malloc(ctx, &b.dev, b.bytes) != hipSuccess) return fail(ctx, VPCC_ERR_DEVICE, "no device memory for digests");
    if (hipHostMalloc(&b.host, b.bytes, hipHostMallocDefault) != hipSuccess) {
      (void)hipFree(b.dev);
      return fail(ctx, VPCC_ERR_DEVICE, "no page-locked memory for digests");
    }
    g->digest.bufs = b;
  }
  g->digest.ctx = ctx;
  if (!g->digest.ready) HIP_TRY(ctx, hipEventCreateWithFlags(&g->digest.ready, hipEventDisableTiming));
  return VPCC_OK;
}

// The stream a gof's digests and test flips go on: behind its latest launch (or its ingest, before the first).
int digest_stream(vpcc_gof* g, hipStream_t* out) {
  vpcc_ctx* ctx = g->ctx;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = g->launched ? g->last_stream : ctx->stream;
  HIP_TRY(ctx, hipStreamWaitEvent(s, g->upload_done, 0));
  *out = s;
  return VPCC_OK;
}

// After work on the gof's outputs or planes: the gof's next launch (on any stream) is ordered behind it.
int digest_done(vpcc_gof* g, hipStream_t s) {
  HIP_TRY(g->ctx, hipGetLastError());
  HIP_TRY(g->ctx, hipEventRecord(g->digest.ready, s));
  if (g->launched) HIP_TRY(g->ctx, hipEventRecord(g->results_ready, s));
  return VPCC_OK;
}

int enqueue_digests(vpcc_gof* g, bool outputs, uint32_t first, uint32_t count, uint32_t slot) {
  if (count == 0 || first >= g->n_frames || count > g->n_frames - first || slot >= kDigestSlots) return VPCC_ERR_INVALID_ARG;
  if (outputs && !g->launched) return fail(g->ctx, VPCC_ERR_STATE, "no reconstruct issued");
  int st = ensure_digest_buffers(g);
  if (st) return st;
  hipStream_t s;
  if ((st = digest_stream(g, &s))) return st;
  unsigned long long* slots = (unsigned long long*)((uint64_t*)g->digest.bufs.dev + (size_t)slot * g->n_frames);
  HIP_TRY(g->ctx, hipMemsetAsync(slots + first, 0, sizeof(uint64_t) * count, s));
  uint64_t bound = 0;                    // word pairs of the largest frame: no more blocks than it can use
  for (uint32_t i = first; i < first + count; ++i) {
    const DevFrame& D = g->h_frames[i];
    bound = std::max<uint64_t>(bound, outputs ? (uint64_t)D.capacity * 9 / 16 + 2 : (uint64_t)D.occ_h + D.map_count * 3ull * D.height);
  }
  const bool timed = (g->flags & VPCC_GOF_PROFILE) != 0;
  if (timed) {
    if (g->digest.timed == g->digest.timing.size()) {
      KernelTiming t{outputs ? "k_digest_outputs" : "k_digest_planes", nullptr, nullptr};
      HIP_TRY(g->ctx, hipEventCreate(&t.start));
      HIP_TRY(g->ctx, hipEventCreate(&t.stop));
      g->digest.timing.push_back(t);
    }
    HIP_TRY(g->ctx, hipEventRecord(g->digest.timing[g->digest.timed].start, s));
  }
  // (planes: a wave per row, four per block; outputs: a lane per word pair)
  const dim3 grid(blocks_per_frame(count, bound, outputs ? kDigestThreads : kDigestThreads / 64), count);
  if (outputs) hipLaunchKernelGGL(k_digest_outputs, grid, dim3(kDigestThreads), 0, s, g->d_frames, first, slots);
  else hipLaunchKernelGGL(k_digest_planes, grid, dim3(kDigestThreads), 0, s, g->d_frames, first, slots);
  if (timed) HIP_TRY(g->ctx, hipEventRecord(g->digest.timing[g->digest.timed++].stop, s));
  return digest_done(g, s);
}

}  // namespace

vpcc_gof::DigestState::~DigestState() {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ready) {
    (void)hipEventSynchronize(ready);
    (void)hipEventDestroy(ready);
  }
  for (auto& t : timing) {
    (void)hipEventDestroy(t.start);
    (void)hipEventDestroy(t.stop);
  }
  if (bufs.dev) {                                      // (hipFree would wait for the whole device)
    if (ctx->digest_cache.size() < 8) ctx->digest_cache.push_back(bufs);
    else { (void)hipFree(bufs.dev); (void)hipHostFree(bufs.host); }
  }
}

namespace vpcc {

int gof_create_check(vpcc_ctx* ctx, const vpcc_frame_desc* frames, uint32_t n_frames, vpcc_gof** out) {
  const int st = vpcc_gof_create(ctx, frames, n_frames, VPCC_MEM_DEVICE, 0, VPCC_GOF_FORCE_GENERAL | VPCC_GOF_PROFILE, out);
  if (st) return st;
  // the general sequence's per-pixel pass on every frame (what VPCC_GENERAL_ANY_FRAME does for a process): no frame of the gof
  // is left to k_general_blocks
  for (vpcc::FrameShape& S : (*out)->shapes) S.block_units = false;
  return VPCC_OK;
}

int gof_enqueue_plane_digests(vpcc_gof* g, uint32_t first, uint32_t count, uint32_t slot) {
  return enqueue_digests(g, false, first, count, slot);
}
int gof_enqueue_output_digests(vpcc_gof* g, uint32_t first, uint32_t count, uint32_t slot) {
  return enqueue_digests(g, true, first, count, slot);
}

int gof_read_digests(vpcc_gof* g, uint64_t* out, double* kernel_seconds) {
  vpcc_ctx* ctx = g->ctx;
  if (kernel_seconds) *kernel_seconds = 0;
  if (!g->digest.bufs.dev) return fail(ctx, VPCC_ERR_STATE, "no digest enqueued");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // on the download stream, like the point counts (fetch_counts): the launch stream may already carry the next units' kernels,
  // which wait for their planes; the slots are PUSHED into page-locked memory by a kernel, not queued behind the copy engines
  hipStream_t s = ctx->d2h_stream;
  HIP_TRY(ctx, hipStreamWaitEvent(s, g->digest.ready, 0));
  const size_t bytes = sizeof(uint64_t) * kDigestSlots * g->n_frames;
  void* dev_host = nullptr;
  if (hipHostGetDevicePointer(&dev_host, g->digest.bufs.host, 0) == hipSuccess && dev_host) {
    IngestPiece pieces[3] = {};
    pieces[0] = IngestPiece{(uint64_t*)g->digest.bufs.dev, dev_host, (uint32_t)bytes, 0u};
    launch_push_results(pieces, s);
    HIP_TRY(ctx, hipGetLastError());
  } else {
    (void)hipGetLastError();
    HIP_TRY(ctx, hipMemcpyAsync(g->digest.bufs.host, (uint64_t*)g->digest.bufs.dev, bytes, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(ctx, hipStreamSynchronize(s));
  std::memcpy(out, g->digest.bufs.host, bytes);
  double sec = 0;
  for (uint32_t i = 0; i < g->digest.timed; ++i) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, g->digest.timing[i].start, g->digest.timing[i].stop) == hipSuccess) sec += ms * 1e-3;
  }
  g->digest.timed = 0;
  if (kernel_seconds) *kernel_seconds = sec;
  return VPCC_OK;
}

int gof_device_plane_desc(vpcc_gof* g, uint32_t frame, vpcc_frame_desc* desc) {
  if (!g || frame >= g->n_frames || !desc) return VPCC_ERR_INVALID_ARG;
  const DevFrame& D = g->h_frames[frame];
  desc->occupancy.y = D.occ;
  desc->occupancy.stride = D.occ_stride;
  for (uint32_t m = 0; m < desc->map_count && m < 2; ++m) {
    desc->geometry[m].y = D.geo[m];
    desc->geometry[m].stride = D.geo_stride[m];
    desc->geometry[m].u = desc->geometry[m].v = nullptr;
    if (!desc->attribute_count) continue;
    desc->attribute[m].y = D.attr_y[m];
    desc->attribute[m].u = D.attr_u[m];
    desc->attribute[m].v = layout_uv(D.layout) ? nullptr : D.attr_v[m];     // (interleaved chroma: the one plane is `u`)
    desc->attribute[m].stride = D.attr_stride[m];
    desc->attribute[m].cstride = D.attr_cstride[m];
  }
  return VPCC_OK;
}

int gof_test_flip_byte(vpcc_gof* g, uint32_t frame, int what) {
  if (!g || frame >= g->n_frames) return VPCC_ERR_INVALID_ARG;
  int st = ensure_digest_buffers(g);
  if (st) return st;
  hipStream_t s;
  if ((st = digest_stream(g, &s))) return st;
  const DevFrame& D = g->h_frames[frame];
  unsigned char* p = what == 0 ? (unsigned char*)const_cast<uint16_t*>(D.geo[0]) : (unsigned char*)D.out_xyz;
  hipLaunchKernelGGL(k_flip_byte, dim3(1), dim3(1), 0, s, p);
  return digest_done(g, s);
}

}  // namespace vpcc

namespace {
int digests_call(vpcc_gof* g, bool outputs, uint32_t first, uint32_t count, uint64_t* out) {
  if (!g || !out) return VPCC_ERR_INVALID_ARG;
  int st = enqueue_digests(g, outputs, first, count, outputs ? kSlotOutputs : kSlotPlanes);
  if (st) return st;
  std::vector<uint64_t> all((size_t)kDigestSlots * g->n_frames);
  if ((st = gof_read_digests(g, all.data(), nullptr))) return st;
  std::memcpy(out, all.data() + (size_t)(outputs ? kSlotOutputs : kSlotPlanes) * g->n_frames + first, sizeof(uint64_t) * count);
  return VPCC_OK;
}
}  // namespace

extern "C" int vpcc_gof_output_digests(vpcc_gof* g, uint32_t first, uint32_t count, uint64_t* out) {
  return digests_call(g, true, first, count, out);
}

extern "C" int vpcc_gof_plane_digests(vpcc_gof* g, uint32_t first, uint32_t count, uint64_t* out) {
  return digests_call(g, false, first, count, out);
}
