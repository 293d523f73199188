// vpcc_digest_host.cpp — the frame digest (include/vpcc_recon.h, "frame digests") on the host: what a caller computes on its
// side to compare with the device's, and what the verified Decoder hashes its input planes and delivered arrays with.
#include <cstring>

#include "vpcc_digest.hpp"

namespace vpcc {

uint64_t digest_row(const void* row, size_t bytes, uint64_t p, uint64_t y) {
  const unsigned char* b = static_cast<const unsigned char*>(row);
  uint64_t s = 0;
  const size_t whole = bytes / 8;
  for (size_t k = 0; k < whole; ++k) {
    uint64_t q;
    std::memcpy(&q, b + 8 * k, 8);                  // little-endian host (x86-64)
    s += digest_term(q, p, y, k);
  }
  if (bytes % 8) {
    uint64_t q = 0;
    std::memcpy(&q, b + 8 * whole, bytes % 8);       // zero-padded at the row's end
    s += digest_term(q, p, y, whole);
  }
  return s;
}

uint64_t digest_frame_planes(const vpcc_frame_desc& f) {
  const uint64_t W = f.width, H = f.height;
  uint64_t s = digest_head((W << 32) | H);
  const vpcc_image_u8& O = f.occupancy;
  for (uint32_t y = 0; y < O.height; ++y) s += digest_row(O.y + (size_t)y * O.stride, O.width, 0, y);
  for (uint32_t m = 0; m < f.map_count && m < 2; ++m) {
    const vpcc_image_u16& G = f.geometry[m];
    for (uint64_t y = 0; y < H; ++y) s += digest_row(G.y + y * G.stride, 2 * W, 1 + m, y);
    if (!f.attribute_count) continue;
    const vpcc_image_u16& A = f.attribute[m];
    for (uint64_t y = 0; y < H; ++y) s += digest_row(A.y + y * A.stride, 2 * W, 3 + 3 * m, y);
    if (f.flags & VPCC_FRAME_UV_INTERLEAVED) {          // one row set of interleaved U,V pairs, as stored
      for (uint64_t y = 0; y < H / 2; ++y) s += digest_row(A.u + y * A.cstride, 4 * (W / 2), 4 + 3 * m, y);
      continue;
    }
    for (uint64_t y = 0; y < H / 2; ++y) s += digest_row(A.u + y * A.cstride, 2 * (W / 2), 4 + 3 * m, y);
    for (uint64_t y = 0; y < H / 2; ++y) s += digest_row(A.v + y * A.cstride, 2 * (W / 2), 5 + 3 * m, y);
  }
  return s;
}

}  // namespace vpcc

extern "C" int vpcc_digest_points(const vpcc_point3* xyz, const vpcc_color3* rgb, size_t n, uint64_t* out) {
  if (!out || (n && !xyz)) return VPCC_ERR_INVALID_ARG;
  uint64_t s = vpcc::digest_head(n) + vpcc::digest_row(xyz, 6 * n, 0, 0);
  if (rgb) s += vpcc::digest_row(rgb, 3 * n, 1, 0);
  *out = s;
  return VPCC_OK;
}

extern "C" int vpcc_digest_frame_planes(const vpcc_frame_desc* f, uint64_t* out) {
  if (!f || !out || f->map_count == 0 || f->map_count > 2 || !f->occupancy.y) return VPCC_ERR_INVALID_ARG;
  if (f->occupancy.stride < f->occupancy.width) return VPCC_ERR_INVALID_ARG;
  for (uint32_t m = 0; m < f->map_count; ++m) {
    const vpcc_image_u16& G = f->geometry[m];
    if (!G.y || G.stride < f->width || G.width < f->width || G.height < f->height) return VPCC_ERR_INVALID_ARG;
    if (!f->attribute_count) continue;
    const vpcc_image_u16& A = f->attribute[m];
    if (f->flags & VPCC_FRAME_UV_INTERLEAVED) {
      if (!A.y || !A.u || A.v || A.stride < f->width || A.cstride < 2 * (f->width / 2) || A.width < f->width || A.height < f->height)
        return VPCC_ERR_INVALID_ARG;
      continue;
    }
    if (!A.y || !A.u || !A.v || A.stride < f->width || A.cstride < f->width / 2 || A.width < f->width || A.height < f->height)
      return VPCC_ERR_INVALID_ARG;
  }
  *out = vpcc::digest_frame_planes(*f);
  return VPCC_OK;
}
