// vpcc_digest.hpp — the frame digest of include/vpcc_recon.h ("frame digests"), shared by the host implementation
// (vpcc_digest_host.cpp), the kernels (vpcc_digest.hip) and the verified Decoder (decoder.cpp).  Internal to libvpcc_recon.so.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "vpcc_recon.h"

#if defined(__HIPCC__)
#define VPCC_DIGEST_FN __host__ __device__ inline
#else
#define VPCC_DIGEST_FN inline
#endif

namespace vpcc {

constexpr uint64_t kDigestG = 0x9E3779B97F4A7C15ull;

VPCC_DIGEST_FN uint64_t mix64(uint64_t z) {
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
// the term of word k of row (p, y)
VPCC_DIGEST_FN uint64_t digest_term(uint64_t q, uint64_t p, uint64_t y, uint64_t k) {
  return mix64(q ^ (((p << 56) | (y << 32) | k) * kDigestG));
}
VPCC_DIGEST_FN uint64_t digest_head(uint64_t head) { return mix64(head ^ kDigestG); }

// Host: Σ_k of one row of `bytes` bytes.
uint64_t digest_row(const void* row, size_t bytes, uint64_t p, uint64_t y);
// Host: the plane digest of frame `f`, whose pointers are host pointers.
uint64_t digest_frame_planes(const vpcc_frame_desc& f);

// The gof side of the verified Decoder (vpcc_digest.hip).  Digests are accumulated in per-gof device slots — kDigestSlots sets
// of n_frames words — enqueued on the gof's launch stream behind its latest kernels, and read back all at once.
enum DigestSlot : uint32_t { kSlotPlanes = 0, kSlotOutputs = 1, kSlotOutputsSmoothed = 2, kDigestSlots = 3 };
int gof_enqueue_plane_digests(vpcc_gof* g, uint32_t first, uint32_t count, uint32_t slot);
int gof_enqueue_output_digests(vpcc_gof* g, uint32_t first, uint32_t count, uint32_t slot);
// Waits for every digest enqueued on the gof (on the download stream: not behind later units' work on the launch stream) and
// copies all slots out: out[slot * n_frames + frame].  *kernel_seconds: HIP-event time of the digest kernels since the last read.
int gof_read_digests(vpcc_gof* g, uint64_t* out, double* kernel_seconds);
// Frame `frame`'s planes as the gof's kernels read them (device pointers and strides): a VPCC_MEM_DEVICE descriptor for a gof
// that borrows them.  `desc` comes in as the frame's original descriptor.
int gof_device_plane_desc(vpcc_gof* g, uint32_t frame, vpcc_frame_desc* desc);
// Tests only (VPCC_DECODER_TEST_CORRUPT): XOR 0x01 into byte 0 of frame `frame`'s geometry plane of map 0 (what = 0) or of its
// positions (what = 1), on the gof's launch stream behind its latest work.
int gof_test_flip_byte(vpcc_gof* g, uint32_t frame, int what);

// The verified Decoder's second reconstruction: a gof over VPCC_MEM_DEVICE planes (borrowed) whose every launch runs the general
// sequence's per-pixel pass (k_general) on every frame — what VPCC_GENERAL_ANY_FRAME does for a whole process.
int gof_create_check(vpcc_ctx* ctx, const vpcc_frame_desc* frames, uint32_t n_frames, vpcc_gof** out);

}  // namespace vpcc
