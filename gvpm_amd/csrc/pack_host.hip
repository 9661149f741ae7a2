// The host codecs of the packed inputs (C ABI, include/gvpm_hip.h): gvpm_pack_* / gvpm_unpack_* for packed and linked photon
// records, packed / compact camera-beam sets, octahedral end normals and run-packed G-VPM samples.  Host only: no handle, no device.  pack_codec.h defines the decode, shared
// with the device decoders (decode_device.hip).
#include <algorithm>
#include <vector>

#include "pack_codec.h"

using namespace gvpm;

namespace {

// unit vector -> octahedral 2 x snorm16 (host)
uint32_t octEncode(const float v[3]) {
  const double x = v[0], y = v[1], z = v[2];
  const double l1 = std::fabs(x) + std::fabs(y) + std::fabs(z);
  if (!(l1 > 0.0) || !std::isfinite(l1)) return GVPM_OCT_ZERO;
  double px = x / l1, py = y / l1;
  if (z < 0.0) {
    const double fx = (1.0 - std::fabs(py)) * (px >= 0.0 ? 1.0 : -1.0), fy = (1.0 - std::fabs(px)) * (py >= 0.0 ? 1.0 : -1.0);
    px = fx;
    py = fy;
  }
  const long ix = std::lrint(px * 32767.0), iy = std::lrint(py * 32767.0);
  return ((uint32_t)(int16_t)ix & 0xFFFFu) | ((uint32_t)(int16_t)iy << 16);
}

// ... the NEAREST code: of the four lattice points around the vector's image, the one whose decode makes the smallest angle
// with it.  Rounding each coordinate (octEncode) is off by up to 6.4e-5 rad in general position -- the third coordinate of the
// decode moves with both -- the nearest code by 4.3e-5.  Same code, same decode; the photon records keep octEncode, whose
// bytes existing blobs and results depend on.
uint32_t octEncodeNearest(const float v[3]) {
  const double x = v[0], y = v[1], z = v[2];
  const double l1 = std::fabs(x) + std::fabs(y) + std::fabs(z), l2 = std::sqrt(x * x + y * y + z * z);
  if (!(l1 > 0.0) || !std::isfinite(l1)) return GVPM_OCT_ZERO;
  double px = x / l1, py = y / l1;
  if (z < 0.0) {
    const double fx = (1.0 - std::fabs(py)) * (px >= 0.0 ? 1.0 : -1.0), fy = (1.0 - std::fabs(px)) * (py >= 0.0 ? 1.0 : -1.0);
    px = fx;
    py = fy;
  }
  const double bx = std::floor(px * 32767.0), by = std::floor(py * 32767.0);
  double bestErr = 1e300;
  long bestX = 0, bestY = 0;
  for (int k = 0; k < 4; ++k) {
    const long ix = std::min(32767L, std::max(-32767L, (long)bx + (k & 1))), iy = std::min(32767L, std::max(-32767L, (long)by + (k >> 1)));
    // octDecode's arithmetic, kept in fp64
    double dx = (double)ix / 32767.0, dy = (double)iy / 32767.0;
    const double dz = 1.0 - std::fabs(dx) - std::fabs(dy);
    if (dz < 0.0) {
      const double fx = (1.0 - std::fabs(dy)) * (dx >= 0.0 ? 1.0 : -1.0), fy = (1.0 - std::fabs(dx)) * (dy >= 0.0 ? 1.0 : -1.0);
      dx = fx;
      dy = fy;
    }
    const double len = std::sqrt(dx * dx + dy * dy + dz * dz);
    const double ex = dx / len - x / l2, ey = dy / len - y / l2, ez = dz / len - z / l2;
    const double err = ex * ex + ey * ey + ez * ez;
    if (err < bestErr) {
      bestErr = err;
      bestX = ix;
      bestY = iy;
    }
  }
  return ((uint32_t)(int16_t)bestX & 0xFFFFu) | ((uint32_t)(int16_t)bestY << 16);
}

// the index of photon i's parent material in `table`, appended if it is new; false: the table is full
// (consecutive photons of a light path mostly share their parent's material: the last hit first)
bool materialIndex(const gvpm_photon_soa &s, uint64_t i, gvpm_material *table, uint32_t &nt, uint32_t cap, uint32_t &last, uint32_t &k) {
  gvpm_material m;
  memcpy(m.scat, s.parent_scat + 3 * i, 12);
  m.g = s.parent_g[i];
  k = last;
  if (!(k < nt && memcmp(&table[k], &m, sizeof(m)) == 0)) {
    for (k = 0; k < nt; ++k)
      if (memcmp(&table[k], &m, sizeof(m)) == 0) break;
    if (k == nt) {
      if (nt >= cap) return false;
      table[nt++] = m;
    }
  }
  last = k;
  return true;
}

// the full 76-byte record of photon i, but for its material
void packFull(const gvpm_photon_soa &s, uint64_t i, gvpm_photon_packed &r) {
  memcpy(r.pos, s.pos + 3 * i, 12);
  memcpy(r.parent_pos, s.parent_pos + 3 * i, 12);
  memcpy(r.flux, s.flux + 3 * i, 12);
  memcpy(r.prefix_w, s.prefix_w + 3 * i, 12);
  r.parent_pdf = s.parent_pdf[i];
  r.edge_pdf = s.edge_pdf[i];
  r.parent_rr = s.parent_rr[i];
  r.parent_n_oct = octEncode(s.parent_n + 3 * i);
  r.parent_wi_oct = octEncode(s.parent_wi + 3 * i);
  r.flags = (s.flags[i] & ~(1u << 7)) | ((s.path_id[i] & 1u) << 7);
}

}  // namespace

// ---- the layout of a blob of linked photon records (include/gvpm_hip.h) ----
static uint64_t align16(uint64_t x) { return (x + 15u) & ~(uint64_t)15u; }
// the offsets of a blob's parts and its size, {kinds, groups, emitters, full, emit, chain, bytes}, in 64 bits: a header
// whose counts need more than its uint32 fields hold is not a blob (linkedHeaderOk)
static void linkedLayout64(const gvpm_linked_header &hd, uint64_t o[7]) {
  uint64_t off = sizeof(gvpm_linked_header);
  o[0] = off;
  off = align16(off + (((uint64_t)hd.n + 15u) / 16u) * 4u);
  o[1] = off;
  off = align16(off + (((uint64_t)hd.n + 63u) / 64u) * 8u);
  o[2] = off;
  off = align16(off + (uint64_t)hd.n_emitters * sizeof(gvpm_emitter_entry));
  o[3] = off;
  off = align16(off + (uint64_t)hd.n_full * sizeof(gvpm_photon_packed));
  o[4] = off;
  off = align16(off + (uint64_t)hd.n_emit * sizeof(gvpm_photon_emit));
  o[5] = off;
  o[6] = align16(off + (uint64_t)hd.n_chain * sizeof(gvpm_photon_chain));
}
// (the packer's blobs: at most 2^25 photons and 1024 emitters, every offset below 2^32)
static void linkedLayout(gvpm_linked_header &hd) {
  uint64_t o[7];
  linkedLayout64(hd, o);
  hd.off_kinds = (uint32_t)o[0];
  hd.off_groups = (uint32_t)o[1];
  hd.off_emitters = (uint32_t)o[2];
  hd.off_full = (uint32_t)o[3];
  hd.off_emit = (uint32_t)o[4];
  hd.off_chain = (uint32_t)o[5];
  hd.bytes = (uint32_t)o[6];
}

// the packer's limit on n, and every offset as the 64-bit layout has it: a uint32 layout wraps for large counts and would
// agree with a header that wrapped the same way
bool gvpm::linkedHeaderOk(const gvpm_linked_header &hd, size_t bytes) {
  if (hd.magic != GVPM_LINKED_MAGIC || hd.n > (1u << 25) || (uint64_t)hd.n_full + hd.n_emit + hd.n_chain != hd.n) return false;
  uint64_t o[7];
  linkedLayout64(hd, o);
  const uint32_t have[7] = {hd.off_kinds, hd.off_groups, hd.off_emitters, hd.off_full, hd.off_emit, hd.off_chain, hd.bytes};
  for (int k = 0; k < 7; ++k)
    if (o[k] != have[k]) return false;
  return (uint64_t)hd.bytes <= (uint64_t)bytes;
}

extern "C" {

int gvpm_pack_photons(const gvpm_photon_soa *src, gvpm_photon_packed *dst, gvpm_material *table, uint32_t table_cap,
                      uint32_t *table_n) {
  if (!src || !table_n || (src->n && (!dst || !table))) return GVPM_ERR_INVALID_ARG;
  if (table_cap > 65536u) table_cap = 65536u;
  uint32_t nt = *table_n, last = 0;
  if (nt > table_cap) return GVPM_ERR_INVALID_ARG;
  for (uint64_t i = 0; i < src->n; ++i) {
    packFull(*src, i, dst[i]);
    if (!materialIndex(*src, i, table, nt, table_cap, last, dst[i].material)) return GVPM_ERR_INVALID_ARG;
  }
  *table_n = nt;
  return GVPM_OK;
}

int gvpm_unpack_photons(const gvpm_photon_packed *src, uint64_t n, const gvpm_material *table, uint32_t table_n,
                        const gvpm_photon_soa *dst) {
  if (!dst || (n && (!src || !dst->pos || !dst->wi || !dst->flux || !dst->parent_pos || !dst->parent_n || !dst->prefix_w ||
                     !dst->parent_scat || !dst->parent_wi || !dst->parent_pdf || !dst->edge_pdf || !dst->parent_rr ||
                     !dst->parent_g || !dst->flags || !dst->path_id)))
    return GVPM_ERR_INVALID_ARG;
  for (uint64_t i = 0; i < n; ++i) {
    if (src[i].material >= table_n) return GVPM_ERR_INVALID_ARG;
    unpackPhoton(src[i], table, table_n, *dst, i);
  }
  return GVPM_OK;
}

// ---- linked photon records (include/gvpm_hip.h) ----
size_t gvpm_linked_photons_bound(uint64_t n) {
  gvpm_linked_header hd{};
  hd.n = hd.n_full = (uint32_t)std::min<uint64_t>(n, 0x3FFFFFFFull);
  hd.n_emitters = 1024u;
  uint64_t o[7];
  linkedLayout64(hd, o);
  return (size_t)o[6] + 64u;
}

int gvpm_pack_photons_linked(const gvpm_photon_soa *src, void *blob, size_t cap, gvpm_material *table, uint32_t table_cap,
                             uint32_t *table_n, size_t *bytes) {
  if (!src || !table_n || !bytes || !blob || (src->n && !table)) return GVPM_ERR_INVALID_ARG;
  const uint64_t n = src->n;
  // 76 B x 2^25 photons keeps every offset below 2^32
  if (n > (1ull << 25)) return GVPM_ERR_INVALID_ARG;
  if (table_cap > 65536u) table_cap = 65536u;
  uint32_t nt = *table_n, lastM = 0, lastE = 0;
  if (nt > table_cap) return GVPM_ERR_INVALID_ARG;
  // pass 1: the kind of every photon (every short kind is VERIFIED against the source), the tables
  std::vector<uint8_t> kind(n, (uint8_t)GVPM_LINKED_FULL);
  std::vector<uint16_t> idx(n, 0);
  std::vector<gvpm_emitter_entry> emitters;
  auto material = [&](uint64_t i, uint32_t &k) { return materialIndex(*src, i, table, nt, table_cap, lastM, k); };
  auto same3 = [](const float *a, const float *b) { return memcmp(a, b, 12) == 0; };
  const float zero3[3] = {0.f, 0.f, 0.f}, ex3[3] = {1.f, 0.f, 0.f};
  uint64_t nf = 0, ne = 0, nc = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t fl = src->flags[i];
    const uint32_t ptype = GVPM_PF_PARENT_TYPE(fl), comp = GVPM_PF_PREV_COMPONENT(fl);
    bool done = false;
    if (i > 0 && ptype == GVPM_PARENT_MEDIUM && comp == (uint32_t)GVPM_BSDF_DIFFUSE_REFLECTION && src->path_id[i] == src->path_id[i - 1] &&
        same3(src->parent_pos + 3 * i, src->pos + 3 * (i - 1)) && same3(src->prefix_w + 3 * i, src->flux + 3 * (i - 1)) &&
        same3(src->parent_n + 3 * i, zero3)) {
      // the link's parent_wi (derived from the two positions before the photon) against the source's: within the octahedral
      // code's error of a full record, or the photon travels as one
      const float *pPrev = src->pos + 3 * (i - 1);
      const float *ppPrev = kind[i - 1] == GVPM_LINKED_CHAIN ? src->pos + 3 * (i - 2) : src->parent_pos + 3 * (i - 1);
      float w[3];
      gvpm::deriveWi(pPrev, ppPrev, w);
      const float *t = src->parent_wi + 3 * i;
      const double cx = (double)w[1] * t[2] - (double)w[2] * t[1], cy = (double)w[2] * t[0] - (double)w[0] * t[2], cz = (double)w[0] * t[1] - (double)w[1] * t[0];
      const double dt = (double)w[0] * t[0] + (double)w[1] * t[1] + (double)w[2] * t[2];
      uint32_t k;
      if (std::sqrt(cx * cx + cy * cy + cz * cz) <= 6e-5 && dt > 0.0) {
        if (!material(i, k)) return GVPM_ERR_INVALID_ARG;
        if (k < 65536u) {
          kind[i] = (uint8_t)GVPM_LINKED_CHAIN;
          idx[i] = (uint16_t)k;
          ++nc;
          done = true;
        }
      }
    }
    if (!done && ptype == GVPM_PARENT_EMITTER && comp == (uint32_t)GVPM_BSDF_DIFFUSE_REFLECTION && same3(src->parent_scat + 3 * i, zero3) &&
        same3(src->parent_wi + 3 * i, ex3)) {
      gvpm_emitter_entry e;
      memcpy(e.prefix_w, src->prefix_w + 3 * i, 12);
      e.parent_rr = src->parent_rr[i];
      memcpy(e.parent_n, src->parent_n + 3 * i, 12);
      e.parent_g = src->parent_g[i];
      uint32_t k = lastE;
      if (!(k < emitters.size() && memcmp(&emitters[k], &e, sizeof(e)) == 0)) {
        for (k = 0; k < emitters.size(); ++k)
          if (memcmp(&emitters[k], &e, sizeof(e)) == 0) break;
        if (k == emitters.size() && k < 1024u) emitters.push_back(e);
      }
      if (k < emitters.size()) {
        lastE = k;
        kind[i] = (uint8_t)GVPM_LINKED_EMIT;
        idx[i] = (uint16_t)k;
        ++ne;
        done = true;
      }
    }
    if (!done) ++nf;
  }
  gvpm_linked_header hd{};
  hd.magic = GVPM_LINKED_MAGIC;
  hd.n = (uint32_t)n;
  hd.n_full = (uint32_t)nf;
  hd.n_emit = (uint32_t)ne;
  hd.n_chain = (uint32_t)nc;
  hd.n_emitters = (uint32_t)emitters.size();
  linkedLayout(hd);
  if ((size_t)hd.bytes > cap) return GVPM_ERR_INVALID_ARG;
  unsigned char *B = static_cast<unsigned char *>(blob);
  memset(B, 0, hd.off_full);
  memcpy(B, &hd, sizeof(hd));
  uint32_t *kinds = reinterpret_cast<uint32_t *>(B + hd.off_kinds);
  uint32_t *groups = reinterpret_cast<uint32_t *>(B + hd.off_groups);
  if (!emitters.empty()) memcpy(B + hd.off_emitters, emitters.data(), emitters.size() * sizeof(gvpm_emitter_entry));
  gvpm_photon_packed *F = reinterpret_cast<gvpm_photon_packed *>(B + hd.off_full);
  gvpm_photon_emit *E = reinterpret_cast<gvpm_photon_emit *>(B + hd.off_emit);
  gvpm_photon_chain *Cn = reinterpret_cast<gvpm_photon_chain *>(B + hd.off_chain);
  uint64_t jf = 0, je = 0, jc = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if ((i & 63u) == 0u) {
      groups[2 * (i >> 6)] = (uint32_t)jf;
      groups[2 * (i >> 6) + 1] = (uint32_t)je;
    }
    kinds[i >> 4] |= (uint32_t)kind[i] << (2u * (uint32_t)(i & 15u));
    const uint32_t lo = (src->flags[i] & 0xFF7Fu) | ((src->path_id[i] & 1u) << 7);
    if (kind[i] == GVPM_LINKED_CHAIN) {
      gvpm_photon_chain &r = Cn[jc++];
      memcpy(r.pos, src->pos + 3 * i, 12);
      memcpy(r.flux, src->flux + 3 * i, 12);
      r.parent_pdf = src->parent_pdf[i];
      r.edge_pdf = src->edge_pdf[i];
      r.parent_rr = src->parent_rr[i];
      r.flags = lo | ((uint32_t)idx[i] << 16);
    } else if (kind[i] == GVPM_LINKED_EMIT) {
      gvpm_photon_emit &r = E[je++];
      memcpy(r.pos, src->pos + 3 * i, 12);
      memcpy(r.parent_pos, src->parent_pos + 3 * i, 12);
      memcpy(r.flux, src->flux + 3 * i, 12);
      r.parent_pdf = src->parent_pdf[i];
      r.edge_pdf = src->edge_pdf[i];
      r.flags = lo | ((uint32_t)idx[i] << 16);
    } else {
      gvpm_photon_packed &r = F[jf++];
      packFull(*src, i, r);
      uint32_t k;
      if (!material(i, k)) return GVPM_ERR_INVALID_ARG;
      r.material = k;
    }
  }
  *table_n = nt;
  *bytes = hd.bytes;
  return GVPM_OK;
}

int gvpm_unpack_photons_linked(const void *blob, size_t bytes, const gvpm_material *table, uint32_t table_n, const gvpm_photon_soa *dst) {
  if (!blob || bytes < sizeof(gvpm_linked_header) || !dst) return GVPM_ERR_INVALID_ARG;
  const unsigned char *B = static_cast<const unsigned char *>(blob);
  gvpm_linked_header hd;
  memcpy(&hd, B, sizeof(hd));
  if (!linkedHeaderOk(hd, bytes)) return GVPM_ERR_INVALID_ARG;
  const uint32_t *kinds = reinterpret_cast<const uint32_t *>(B + hd.off_kinds);
  const gvpm_emitter_entry *emitters = reinterpret_cast<const gvpm_emitter_entry *>(B + hd.off_emitters);
  const gvpm_photon_packed *F = reinterpret_cast<const gvpm_photon_packed *>(B + hd.off_full);
  const gvpm_photon_emit *E = reinterpret_cast<const gvpm_photon_emit *>(B + hd.off_emit);
  const gvpm_photon_chain *Cn = reinterpret_cast<const gvpm_photon_chain *>(B + hd.off_chain);
  const uint32_t *groups = reinterpret_cast<const uint32_t *>(B + hd.off_groups);
  uint64_t jf = 0, je = 0, jc = 0;
  for (uint64_t i = 0; i < hd.n; ++i) {
    // the per-64-photon bases the device indexes with ARE the running counts (the device checks the same per group)
    if ((i & 63u) == 0u && (groups[2 * (i >> 6)] != jf || groups[2 * (i >> 6) + 1] != je)) return GVPM_ERR_INVALID_ARG;
    const uint32_t k = gvpm::linkedKind(kinds, i);
    if (k == GVPM_LINKED_FULL) {
      if (jf >= hd.n_full || F[jf].material >= table_n) return GVPM_ERR_INVALID_ARG;
      gvpm::unpackPhoton(F[jf++], table, table_n, *dst, i);
    } else if (k == GVPM_LINKED_EMIT) {
      if (je >= hd.n_emit || (E[je].flags >> 16) >= hd.n_emitters) return GVPM_ERR_INVALID_ARG;
      gvpm::unpackEmit(E[je++], emitters, hd.n_emitters, *dst, i);
    } else if (k == GVPM_LINKED_CHAIN) {
      if (jc >= hd.n_chain || i == 0 || (Cn[jc].flags >> 16) >= table_n) return GVPM_ERR_INVALID_ARG;
      gvpm::unpackChainOwn(Cn[jc++], table, table_n, *dst, i);
    } else {
      return GVPM_ERR_INVALID_ARG;
    }
  }
  for (uint64_t i = 1; i < hd.n; ++i)
    if (gvpm::linkedKind(kinds, i) == GVPM_LINKED_CHAIN) gvpm::linkChain(*dst, i, i >= 2 && gvpm::linkedKind(kinds, i - 1) == GVPM_LINKED_CHAIN);
  return GVPM_OK;
}

int gvpm_pack_camera_beams(const gvpm_camera_ray *rays, uint64_t n_sets, gvpm_beam_set_packed *dst) {
  if (n_sets && (!rays || !dst)) return GVPM_ERR_INVALID_ARG;
  for (uint64_t i = 0; i < n_sets; ++i) {
    const gvpm_camera_ray *s = rays + 5 * i;
    dst[i].base = s[0];
    for (int k = 1; k < 5; ++k) {
      if (GVPM_RAY_EDGE(s[k].info) != GVPM_RAY_EDGE(s[0].info)) return GVPM_ERR_INVALID_ARG;
      gvpm_ray_packed &q = dst[i].shifted[k - 1];
      for (int c = 0; c < 3; ++c) {
        q.o[c] = s[k].o[c];
        q.d[c] = s[k].d[c];
        q.eye[c] = s[k].eye[c];
      }
      const float l = std::fabs(s[k].len);
      q.len = GVPM_RAY_VALID(s[k].info) ? l : -l;  // (the sign BIT: -0 is an invalid ray of length 0)
      q.pdf = s[k].pdf;
      q.jacobian = s[k].jacobian;
      q.gop = s[k].gop;
    }
  }
  return GVPM_OK;
}

int gvpm_unpack_camera_beams(const gvpm_beam_set_packed *src, uint64_t n_sets, gvpm_camera_ray *dst) {
  if (n_sets && (!src || !dst)) return GVPM_ERR_INVALID_ARG;
  for (uint64_t i = 0; i < n_sets; ++i)
    for (int k = 0; k < 5; ++k) dst[5 * i + k] = unpackRay(src[i], k);
  return GVPM_OK;
}

// ---- the side inputs of the beam / plane / G-VPM techniques (include/gvpm_hip.h) ----
int gvpm_pack_normals_oct(const float *normals, uint64_t n, uint32_t *codes) {
  if (n && (!normals || !codes)) return GVPM_ERR_INVALID_ARG;
  for (uint64_t i = 0; i < n; ++i) codes[i] = octEncodeNearest(normals + 3 * i);
  return GVPM_OK;
}

int gvpm_unpack_normals_oct(const uint32_t *codes, uint64_t n, float *normals) {
  if (n && (!codes || !normals)) return GVPM_ERR_INVALID_ARG;
  for (uint64_t i = 0; i < n; ++i) octDecode(codes[i], normals + 3 * i);
  return GVPM_OK;
}

int gvpm_pack_vpm_samples(const gvpm_vpm_sample *samples, uint64_t n, gvpm_vpm_run *runs, uint64_t runs_cap, uint64_t *n_runs,
                          float *rands) {
  if (!n_runs || n > 0x7FFFFFF0ull || (n && (!samples || !runs || !rands))) return GVPM_ERR_INVALID_ARG;
  uint64_t nr = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const gvpm_vpm_sample &s = samples[i];
    if (s.reserved != 0u) return GVPM_ERR_INVALID_ARG;
    // (bit-equal: -0 and 0, or two NaNs, are not one run -- the decode must give back the bytes)
    const bool same = nr > 0 && runs[nr - 1].set == s.set && memcmp(&runs[nr - 1].pdf_sel, &s.pdf_sel, 4) == 0;
    if (same) {
      runs[nr - 1].count++;
    } else {
      if (nr >= runs_cap) return GVPM_ERR_INVALID_ARG;
      runs[nr++] = gvpm_vpm_run{s.set, s.pdf_sel, (uint32_t)i, 1u};
    }
    rands[i] = s.rand;
  }
  *n_runs = nr;
  return GVPM_OK;
}

int gvpm_unpack_vpm_samples(const gvpm_vpm_run *runs, uint64_t n_runs, const float *rands, uint64_t n, gvpm_vpm_sample *dst) {
  if (n > 0x7FFFFFF0ull || (n && (!rands || !dst)) || !vpmRunsOk(runs, n_runs, n)) return GVPM_ERR_INVALID_ARG;
  for (uint64_t i = 0; i < n; ++i) dst[i] = expandVpmSample(runs, (uint32_t)n_runs, rands, (uint32_t)i);
  return GVPM_OK;
}

int gvpm_unpack_camera_beams_compact(const gvpm_sensor *sensor, const gvpm_beam_set_compact *src, uint64_t n_compact,
                                     gvpm_camera_ray *dst) {
  if (!sensor || (n_compact && (!src || !dst))) return GVPM_ERR_INVALID_ARG;
  for (uint64_t i = 0; i < n_compact; ++i)
    for (int k = 0; k < 5; ++k) dst[5 * i + k] = unpackCompactRay(*sensor, src[i], k);
  return GVPM_OK;
}

int gvpm_pack_camera_beams_compact(const gvpm_sensor *sensor, const gvpm_camera_ray *rays, const float *jitter,
                                   uint64_t n_sets, gvpm_beam_set_compact *compact, uint64_t *n_compact,
                                   gvpm_beam_set_packed *full, uint64_t *n_full, uint32_t *new_index) {
  if (!sensor || !n_compact || !n_full || (n_sets && (!rays || !jitter || !compact || !full))) return GVPM_ERR_INVALID_ARG;
  uint64_t nc = 0, nf = 0;
  std::vector<uint8_t> isFull(new_index ? n_sets : 0);
  for (uint64_t i = 0; i < n_sets; ++i) {
    const gvpm_camera_ray *s = rays + 5 * i;
    gvpm_beam_set_compact c;
    memset(&c, 0, sizeof(c));
    c.pixel = s[0].pixel;
    c.jitter[0] = jitter[2 * i];
    c.jitter[1] = jitter[2 * i + 1];
    c.rand = s[0].rand;
    const uint32_t edge = GVPM_RAY_EDGE(s[0].info);
    c.info = edge << 8;
    bool ok = c.jitter[0] >= 0.f && c.jitter[0] < 1.f && c.jitter[1] >= 0.f && c.jitter[1] < 1.f;
    for (int k = 0; k < 5; ++k) {
      if (GVPM_RAY_EDGE(s[k].info) != edge) return GVPM_ERR_INVALID_ARG;
      if (!GVPM_RAY_VALID(s[k].info)) continue;
      c.info |= 1u << k;
      const double ox = (double)s[k].o[0] - sensor->pos[0], oy = (double)s[k].o[1] - sensor->pos[1], oz = (double)s[k].o[2] - sensor->pos[2];
      // (a ray that starts AT the sensor -- the sensor sits in the medium -- has t0 = 0 whatever the rounding of pos)
      const bool atSensor = (float)sensor->pos[0] == s[k].o[0] && (float)sensor->pos[1] == s[k].o[1] && (float)sensor->pos[2] == s[k].o[2];
      c.t0[k] = atSensor ? 0.f : (float)std::sqrt(ox * ox + oy * oy + oz * oz);
      c.len[k] = s[k].len;
    }
    // eligible iff the decode gives the rays back (to rounding) and the fields the format drops hold what it assumes
    for (int k = 0; k < 5 && ok; ++k) {
      const gvpm_camera_ray u = unpackCompactRay(*sensor, c, k);
      if (u.info != s[k].info) ok = false;
      if (!GVPM_RAY_VALID(s[k].info)) continue;
      for (int a = 0; a < 3 && ok; ++a) {
        const double tolD = 4.0 * 1.1920929e-7, tolO = 4.0 * 1.1920929e-7 * std::fmax(1.0, std::fabs((double)s[k].o[a]));
        if (std::fabs((double)u.d[a] - (double)s[k].d[a]) > tolD || std::fabs((double)u.o[a] - (double)s[k].o[a]) > tolO) ok = false;
        if (s[k].eye[a] != 1.f) ok = false;
      }
      if (u.len != s[k].len) ok = false;
      if (k > 0 && ok) {
        const double prod = (double)s[k].pdf / (double)s[0].pdf * (double)s[k].jacobian;
        if (!(std::fabs(prod - 1.0) <= 1e-4)) ok = false;
      }
    }
    if (ok && (!GVPM_RAY_VALID(s[0].info))) ok = false;  // (a set without a base ray is not a set)
    if (ok) {
      compact[nc++] = c;
    } else {
      const int rc = gvpm_pack_camera_beams(s, 1, full + nf);
      if (rc != GVPM_OK) return rc;
      ++nf;
    }
    if (new_index) isFull[i] = !ok;
  }
  if (new_index) {
    uint64_t a = 0, b = nc;
    for (uint64_t i = 0; i < n_sets; ++i) new_index[i] = (uint32_t)(isFull[i] ? b++ : a++);
  }
  *n_compact = nc;
  *n_full = nf;
  return GVPM_OK;
}

}  // extern "C"
