// host_crc.inc -- zlib's CRC-32 of device memory (kernels_crc.hpp): the plan, the two launches, and the join of pieces on the host.

extern "C" uint64_t scalce_crc32_ws_bytes(uint64_t nbytes) {
  (void)nbytes;  // one word per workgroup, and the grid has a fixed bound
  return sizeof(u32) * CRC_MAX_WG;
}

extern "C" int scalce_crc32_plan(uint64_t nbytes, uint32_t out[4]) {
  CrcPlan p;
  if (!out || !crc_plan(0, nbytes, &p)) return SCALCE_ERR_ARG;
  out[0] = CRC_GRANULE;
  out[1] = CRC_TILE;
  out[2] = p.span;
  out[3] = p.wgs;
  return SCALCE_OK;
}

extern "C" uint32_t scalce_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
  return scalce_host::crc32_combine(crc_a, crc_b, len_b);
}

extern "C" int scalce_crc32_device(scalce_ctx *c, const uint8_t *d_data, uint64_t nbytes, uint32_t *d_crc, void *ws, void *stream) {
  if (!c) return SCALCE_ERR_ARG;
  if (!d_crc || !ws || (nbytes && !d_data) || nbytes > CRC_MAX_BYTES) {
    set_err(c, "scalce_crc32_device: bad argument");
    return SCALCE_ERR_ARG;
  }
  static const scalce_host::CrcPowers powers = scalce_host::crc_powers();
  hipStream_t s = (hipStream_t)stream;
  const u64 head = nbytes ? (u64)(reinterpret_cast<uintptr_t>(d_data) & (CRC_GRANULE - 1)) : 0;
  CrcPlan p;
  crc_plan(head, nbytes, &p);
  CrcArgs a;
  a.base = d_data - head;
  a.lo = head;
  a.hi = head + nbytes;
  a.tiles_per_span = p.tile_count_per_span;
  a.partial = static_cast<u32 *>(ws);
  a.out = d_crc;
  a.nwg = p.wgs;
  a.pw = powers;
  HIP_TRY(c, hipSetDevice(c->device));
  if (p.wgs) {
    HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void *>(crc32_span_k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)CRC_LDS_BYTES));
    LAUNCH(crc32_span_k, p.wgs, CRC_THREADS, CRC_LDS_BYTES, s, a);
  }
  LAUNCH(crc32_join_k, 1, 256, 0, s, a);
  return launch_failed(c);
}
