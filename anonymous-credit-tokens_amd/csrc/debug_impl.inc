// debug_impl.inc -- test hooks, roofline probes and kernel timing behind the C ABI (included by engine.hip, inside its extern "C"
// block): act_debug_*, act_ubench_*, act_prof_*.  Nothing here is on the product's path.
int act_debug_last_spend_transcripts(act_ctx* c, size_t max_lanes, uint8_t* out, size_t* n_copied) {
  if (!c || !out || !n_copied) return ACT_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCK(c, hipSetDevice(c->device));
  const SpendTranscript st{c->L};
  Slot& sl = c->slots[c->last_spend_slot];
  size_t m = std::min(max_lanes, sl.last_spend_lanes);
  std::vector<uint8_t> tmp(m * st.stride());
  HIPCK(c, hipMemcpy(tmp.data(), sl.d_tr, tmp.size(), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < m; i++) memcpy(out + i * st.bytes(), tmp.data() + i * st.stride(), st.bytes());
  *n_copied = m;
  return ACT_OK;
}

// v_mad_u64_u32 issue-rate micro-benchmark (k_misc.hip k_ubench_mad): the ALU roofline of this arithmetic, measured on the
// GPU and in the process that runs the workload.  lane_mads_per_s = 64-bit multiply-accumulates per second summed over lanes.
int act_ubench_mad_u64_u32(int device, double* lane_mads_per_s, double* ms) {
  if (!lane_mads_per_s) return ACT_ERR_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return ACT_ERR_NO_DEVICE;
  if (device < 0 || device >= ndev || hipSetDevice(device) != hipSuccess) return ACT_ERR_ARG;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return ACT_ERR_HIP;
  const int iters_env = (int)tune(T_UBENCH_ITERS);        // measurement knob: probe length
  // 8 blocks x 4 waves per CU: 8 waves per SIMD.  Long enough (~0.3 s) for the clock to settle where a sustained ALU load
  // leaves it (the measured rate rises from 2.8e13 over 6 ms to 3.49e13 over 0.3 s and stays there)
  const uint32_t blocks = (uint32_t)prop.multiProcessorCount * 8u, iters = iters_env > 0 ? (uint32_t)iters_env : 262144u;
  uint32_t* d = nullptr; hipEvent_t e0, e1; hipStream_t st;
  int rc = ACT_OK; float t = 0;
  if (hipMalloc(&d, (size_t)blocks * 256 * 4) != hipSuccess) return ACT_ERR_HIP;
  if (hipStreamCreate(&st) != hipSuccess || hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { (void)hipFree(d); return ACT_ERR_HIP; }
  launch_ubench_mad(d, blocks, iters / 16, st);                               // warm-up (clocks, code load)
  (void)hipEventRecord(e0, st);
  launch_ubench_mad(d, blocks, iters, st);
  (void)hipEventRecord(e1, st);
  if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&t, e0, e1) != hipSuccess) rc = ACT_ERR_HIP;
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipStreamDestroy(st); (void)hipFree(d);
  if (rc) { (void)hipGetLastError(); return rc; }
  *lane_mads_per_s = (double)blocks * 256.0 * iters * UBENCH_MADS_PER_ITER / (t * 1e-3);
  if (ms) *ms = t;
  return ACT_OK;
}

// 128-byte random-read micro-benchmark (k_misc.hip k_ubench_random_read): the memory-side roofline of the scalar-addressed
// fixed-base tables.  `gib` GiB of device memory are allocated for the probe and freed again (0 = 16); waves_per_simd (0 = 2) and
// in_flight (1, 2 or 4; 0 = 2) set how many lines a CU has outstanding.
static int ubench_random_read_impl(int device, const uint32_t* table, size_t table_bytes, size_t gib, int waves_per_simd, int in_flight, double* gbytes_per_s, double* ms) {
  if (!gbytes_per_s) return ACT_ERR_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return ACT_ERR_NO_DEVICE;
  if (device < 0 || device >= ndev || hipSetDevice(device) != hipSuccess) return ACT_ERR_ARG;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return ACT_ERR_HIP;
  size_t bytes;
  if (table) { bytes = (size_t)1 << 20; while (bytes * 2 <= table_bytes) bytes *= 2; }      // the largest power-of-two prefix of the table
  else { size_t g2 = 1; while (g2 * 2 <= (gib ? gib : 16)) g2 *= 2; bytes = g2 << 30; }     // a power of two: the kernel masks its line numbers
  const uint64_t lines = bytes / 128;
  if (waves_per_simd <= 0) waves_per_simd = 2;
  if (waves_per_simd > 8) waves_per_simd = 8;
  if (in_flight <= 0) in_flight = 2;
  const uint32_t blocks = (uint32_t)prop.multiProcessorCount * (uint32_t)waves_per_simd, iters = 4096u * 8u / (uint32_t)waves_per_simd;
  uint32_t *buf = const_cast<uint32_t*>(table), *out = nullptr; hipEvent_t e0, e1; hipStream_t st;
  if (!table && hipMalloc(&buf, bytes) != hipSuccess) { (void)hipGetLastError(); return ACT_ERR_HIP; }
  if (hipMalloc(&out, (size_t)blocks * 256 * 4) != hipSuccess) { (void)hipGetLastError(); if (!table) (void)hipFree(buf); return ACT_ERR_HIP; }
  int rc = ACT_OK; float t = 0;
  if (hipStreamCreate(&st) != hipSuccess || hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { if (!table) (void)hipFree(buf); (void)hipFree(out); return ACT_ERR_HIP; }
  if (!table) (void)hipMemsetAsync(buf, 0x5a, bytes, st);                      // touch every page
  launch_ubench_random_read(buf, lines, blocks, 64, in_flight, out, st);       // warm-up
  (void)hipEventRecord(e0, st);
  launch_ubench_random_read(buf, lines, blocks, iters, in_flight, out, st);
  (void)hipEventRecord(e1, st);
  if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&t, e0, e1) != hipSuccess) rc = ACT_ERR_HIP;
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipStreamDestroy(st); if (!table) (void)hipFree(buf); (void)hipFree(out);
  if (rc) { (void)hipGetLastError(); return rc; }
  *gbytes_per_s = (double)blocks * 256.0 * iters * 128.0 / (t * 1e-3) / 1e9;     // a 128-byte line per read (112 bytes of it used, as the tables' entries)
  if (ms) *ms = t;
  return ACT_OK;
}
int act_ubench_random_read(int device, size_t gib, int waves_per_simd, int in_flight, double* gbytes_per_s, double* ms) {
  return ubench_random_read_impl(device, nullptr, 0, gib, waves_per_simd, in_flight, gbytes_per_s, ms);
}
// the same probe on the context's OWN table of `base` (0..3 = g, h1, h2, h3): the product's entries in the product's memory, read
// in the product's pattern with nothing else going on -- the ceiling of fixed_base_acc's look-ups as this context has them
int act_ubench_table_read(act_ctx* c, int base, int waves_per_simd, int in_flight, double* gbytes_per_s, double* ms) {
  if (!c || base < 0 || base > 3) return ACT_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  return ubench_random_read_impl(c->device, c->d_tables[base], fb_table_words((uint32_t)c->fb_bits[base]) * 4, 0, waves_per_simd, in_flight, gbytes_per_s, ms);
}

int act_debug_scalarmult_batch(act_ctx* c, size_t n, int mem, const uint8_t* points, const uint8_t* scalars, uint8_t* out, uint8_t* status) {
  if (!c || (n && (!points || !scalars || !out || !status))) return ACT_ERR_ARG;
  Call call(c, n);
  HIPCK(c, hipSetDevice(c->device));
  Slot& sl = c->slots[0];
  for (size_t off = 0; off < n; off += c->max_batch) {
    uint32_t m = (uint32_t)std::min(c->max_batch, n - off);
    const uint8_t *d_p, *d_s; uint8_t* d_o; int rc;
    if ((rc = dev_in(c, sl, 0, mem, points + off * 32, (size_t)m * 32, &d_p))) return rc;
    if ((rc = dev_in(c, sl, 1, mem, scalars + off * 32, (size_t)m * 32, &d_s))) return rc;
    if ((rc = dev_out_begin(c, sl, 2, mem, out + off * 32, (size_t)m * 32, &d_o))) return rc;
    launch_debug_scalarmult(d_p, d_s, m, sl.d_buckets, d_o, sl.d_status, sl.stream);
    if ((rc = dev_out_end(c, sl, mem, out + off * 32, d_o, (size_t)m * 32))) return rc;
    if ((rc = copy_status_out(c, sl, mem, status + off, m))) return rc;
    HIPCK(c, hipStreamSynchronize(sl.stream));
  }
  return call.finish();
}

// out[i] = enc(scalars[i] * B), B = base 0..3 (g, h1, h2, h3), through fixed_base_acc on the table and window width the context holds
// for B at this moment (act_ctx_set_fixed_base_bits)
int act_debug_fixed_base_batch(act_ctx* c, int base, size_t n, int mem, const uint8_t* scalars, uint8_t* out) {
  if (!c || base < 0 || base > 3 || (n && (!scalars || !out))) return ACT_ERR_ARG;
  Call call(c, n);
  HIPCK(c, hipSetDevice(c->device));
  Slot& sl = c->slots[0];
  for (size_t off = 0; off < n; off += c->max_batch) {
    uint32_t m = (uint32_t)std::min(c->max_batch, n - off);
    const uint8_t* d_s; uint8_t* d_o; int rc;
    if ((rc = dev_in(c, sl, 0, mem, scalars + off * 32, (size_t)m * 32, &d_s))) return rc;
    if ((rc = dev_out_begin(c, sl, 1, mem, out + off * 32, (size_t)m * 32, &d_o))) return rc;
    launch_debug_fixed_base(c->P.tab[base], d_s, m, d_o, sl.stream);
    if ((rc = dev_out_end(c, sl, mem, out + off * 32, d_o, (size_t)m * 32))) return rc;
    HIPCK(c, hipStreamSynchronize(sl.stream));
  }
  return call.finish();
}

// One field operation per lane on raw limbs (k_debug_fe.hip), in the per-column build of fe25519.h or in the range kernel's
// (pair_build).  h / hb go IN as well, rounded up to whole blocks of 256 lanes, and come back whole: a lane from n on that the kernel
// wrote would show in what the caller pre-filled.
int act_debug_fe_batch(act_ctx* c, int pair_build, int op, size_t n, const uint32_t* f, const uint32_t* g, const uint32_t* fb, const uint32_t* gb_or_a, uint32_t* h, uint32_t* hb) {
  if (!c || op < 0 || op >= DFE_COUNT) return ACT_ERR_ARG;
  const bool two = op == DFE_MUL2 || op == DFE_SQ2 || op == DFE_SQDA_SQ;
  const bool need_g = op == DFE_MUL || op == DFE_MUL2 || op == DFE_SUB || op == DFE_SUB3 || op == DFE_SUB4, need_ga = op == DFE_MUL2 || op == DFE_SQDA_SQ;
  if (n && (!f || !h || (need_g && !g) || (two && (!fb || !hb)) || (need_ga && !gb_or_a))) return ACT_ERR_ARG;
  Call call(c, n);
  HIPCK(c, hipSetDevice(c->device));
  Slot& sl = c->slots[0];
  const size_t LB = FE_LIMBS * 4;                                   // bytes of a lane
  const size_t chunk = std::max<size_t>(256, c->max_batch / 256 * 256);      // whole blocks
  for (size_t off = 0; off < n; off += chunk) {
    const uint32_t m = (uint32_t)std::min(chunk, n - off);
    const size_t in_b = (size_t)m * LB, out_b = ((size_t)m + 255) / 256 * 256 * LB;
    const uint8_t *d_f, *d_g = nullptr, *d_fb = nullptr, *d_ga = nullptr, *d_hin, *d_hbin = nullptr; uint8_t *d_h, *d_hb = nullptr; int rc;
    if ((rc = dev_in(c, sl, 0, ACT_MEM_HOST, (const uint8_t*)f + off * LB, in_b, &d_f))) return rc;
    if (need_g && (rc = dev_in(c, sl, 1, ACT_MEM_HOST, (const uint8_t*)g + off * LB, in_b, &d_g))) return rc;
    if (two && (rc = dev_in(c, sl, 2, ACT_MEM_HOST, (const uint8_t*)fb + off * LB, in_b, &d_fb))) return rc;
    if (need_ga && (rc = dev_in(c, sl, 3, ACT_MEM_HOST, (const uint8_t*)gb_or_a + off * LB, in_b, &d_ga))) return rc;
    if ((rc = dev_in(c, sl, 4, ACT_MEM_HOST, (const uint8_t*)h + off * LB, out_b, &d_hin))) return rc;
    if (two && (rc = dev_in(c, sl, 5, ACT_MEM_HOST, (const uint8_t*)hb + off * LB, out_b, &d_hbin))) return rc;
    d_h = const_cast<uint8_t*>(d_hin); d_hb = const_cast<uint8_t*>(d_hbin);
    (pair_build ? launch_debug_fe_pair : launch_debug_fe)(op, m, (const uint32_t*)d_f, (const uint32_t*)d_g, (const uint32_t*)d_fb, (const uint32_t*)d_ga, (uint32_t*)d_h, (uint32_t*)d_hb, sl.stream);
    HIPCK(c, hipGetLastError());
    if ((rc = dev_out_end(c, sl, ACT_MEM_HOST, (uint8_t*)h + off * LB, d_h, out_b))) return rc;
    if (two && (rc = dev_out_end(c, sl, ACT_MEM_HOST, (uint8_t*)hb + off * LB, d_hb, out_b))) return rc;
    HIPCK(c, hipStreamSynchronize(sl.stream));
  }
  return call.finish();
}

// One operation of the scalar arithmetic mod l per lane (k_debug_sc.hip) on records of DSC_WORDS words.  r goes IN as well, rounded up
// to whole blocks of 256 lanes, and comes back whole, as h does above: a word the kernel wrote past its result, or past lane n, shows
// in what the caller pre-filled.
int act_debug_sc_batch(act_ctx* c, int op, size_t n, const uint32_t* a, const uint32_t* b, const uint32_t* c3, uint32_t* r) {
  if (!c || op < 0 || op >= DSC_COUNT) return ACT_ERR_ARG;
  const bool need_b = op == DSC_ADD || op == DSC_SUB || op == DSC_MUL || op == DSC_MULADD || op == DSC_SCM_MUL || op == DSC_EQUAL, need_c = op == DSC_MULADD;
  if (n && (!a || !r || (need_b && !b) || (need_c && !c3))) return ACT_ERR_ARG;
  Call call(c, n);
  HIPCK(c, hipSetDevice(c->device));
  Slot& sl = c->slots[0];
  const size_t LB = DSC_WORDS * 4;                                  // bytes of a lane's record
  const size_t chunk = std::max<size_t>(256, c->max_batch / 256 * 256);      // whole blocks
  for (size_t off = 0; off < n; off += chunk) {
    const uint32_t m = (uint32_t)std::min(chunk, n - off);
    const size_t in_b = (size_t)m * LB, out_b = ((size_t)m + 255) / 256 * 256 * LB;
    const uint8_t *d_a, *d_b = nullptr, *d_c = nullptr, *d_rin; int rc;
    if ((rc = dev_in(c, sl, 0, ACT_MEM_HOST, (const uint8_t*)a + off * LB, in_b, &d_a))) return rc;
    if (need_b && (rc = dev_in(c, sl, 1, ACT_MEM_HOST, (const uint8_t*)b + off * LB, in_b, &d_b))) return rc;
    if (need_c && (rc = dev_in(c, sl, 2, ACT_MEM_HOST, (const uint8_t*)c3 + off * LB, in_b, &d_c))) return rc;
    if ((rc = dev_in(c, sl, 3, ACT_MEM_HOST, (const uint8_t*)r + off * LB, out_b, &d_rin))) return rc;
    uint8_t* d_r = const_cast<uint8_t*>(d_rin);
    launch_debug_sc(op, m, (const uint32_t*)d_a, (const uint32_t*)d_b, (const uint32_t*)d_c, (uint32_t*)d_r, sl.stream);
    HIPCK(c, hipGetLastError());
    if ((rc = dev_out_end(c, sl, ACT_MEM_HOST, (uint8_t*)r + off * LB, d_r, out_b))) return rc;
    HIPCK(c, hipStreamSynchronize(sl.stream));
  }
  return call.finish();
}

// out[i] = enc(scalars[i] * B), B = base 0..3, through the product of SECRET scalars: fixed_base_acc_mf over the context's own
// matrix-core table image of B (k_debug_secret.hip), in blocks of 64 or 256 threads.  Chunked by max_batch as the hook above is; lane
// i of a chunk is thread i of the launch, so with max_batch a multiple of 64 scalar i sits in lane i mod 64 of its wavefront.
int act_debug_fixed_base_mf_batch(act_ctx* c, int base, int block_threads, size_t n, int mem, const uint8_t* scalars, uint8_t* out) {
  if (!c || base < 0 || base > 3 || (block_threads != 64 && block_threads != 256) || (n && (!scalars || !out))) return ACT_ERR_ARG;
  Call call(c, n);
  HIPCK(c, hipSetDevice(c->device));
  Slot& sl = c->slots[0];
  for (size_t off = 0; off < n; off += c->max_batch) {
    uint32_t m = (uint32_t)std::min(c->max_batch, n - off);
    const uint8_t* d_s; uint8_t* d_o; int rc;
    if ((rc = dev_in(c, sl, 0, mem, scalars + off * 32, (size_t)m * 32, &d_s))) return rc;
    if ((rc = dev_out_begin(c, sl, 1, mem, out + off * 32, (size_t)m * 32, &d_o))) return rc;
    launch_debug_fixed_base_mf(c->P.tab_mf[base], block_threads, d_s, m, d_o, sl.stream);
    HIPCK(c, hipGetLastError());
    if ((rc = dev_out_end(c, sl, mem, out + off * 32, d_o, (size_t)m * 32))) return rc;
    HIPCK(c, hipStreamSynchronize(sl.stream));
  }
  return call.finish();
}

// The address-free variable-base chains, one per lane (k_debug_secret.hip): mode 0 out = enc(s P) by chain_ct<1>, 1 the same from the
// four chain_ct_quarter pieces, 2 out = enc(s P) and out2 = enc(s2 P) by chain_ct<2>.  status 255 and zero records for a point that
// does not decode.  scalars2 / out2 are read and written in mode 2 only.
int act_debug_chain_ct_batch(act_ctx* c, int mode, size_t n, int mem, const uint8_t* points, const uint8_t* scalars, const uint8_t* scalars2, uint8_t* out, uint8_t* out2, uint8_t* status) {
  if (!c || mode < 0 || mode > 2 || (n && (!points || !scalars || !out || !status || (mode == 2 && (!scalars2 || !out2))))) return ACT_ERR_ARG;
  Call call(c, n);
  HIPCK(c, hipSetDevice(c->device));
  Slot& sl = c->slots[0];
  for (size_t off = 0; off < n; off += c->max_batch) {
    uint32_t m = (uint32_t)std::min(c->max_batch, n - off);
    const size_t b = (size_t)m * 32;
    const uint8_t *d_p, *d_s, *d_s2 = nullptr; uint8_t *d_o, *d_o2 = nullptr; int rc;
    if ((rc = dev_in(c, sl, 0, mem, points + off * 32, b, &d_p))) return rc;
    if ((rc = dev_in(c, sl, 1, mem, scalars + off * 32, b, &d_s))) return rc;
    if (mode == 2 && (rc = dev_in(c, sl, 2, mem, scalars2 + off * 32, b, &d_s2))) return rc;
    if ((rc = dev_out_begin(c, sl, 3, mem, out + off * 32, b, &d_o))) return rc;
    if (mode == 2 && (rc = dev_out_begin(c, sl, 4, mem, out2 + off * 32, b, &d_o2))) return rc;
    launch_debug_chain_ct(mode, d_p, d_s, d_s2, m, d_o, d_o2, sl.d_status, sl.stream);
    HIPCK(c, hipGetLastError());
    if ((rc = dev_out_end(c, sl, mem, out + off * 32, d_o, b))) return rc;
    if (mode == 2 && (rc = dev_out_end(c, sl, mem, out2 + off * 32, d_o2, b))) return rc;
    if ((rc = copy_status_out(c, sl, mem, status + off, m))) return rc;
    HIPCK(c, hipStreamSynchronize(sl.stream));
  }
  return call.finish();
}

// Test hook: bytes that are not zero in the context's secret-bearing buffers (what finish_call wipes), read back to the host.
int act_debug_secret_residue(act_ctx* c, size_t* nonzero_bytes) {
  if (!c || !nonzero_bytes) return ACT_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  HIPCK(c, hipSetDevice(c->device));
  size_t total = 0, nz = 0;
  std::vector<std::pair<const void*, size_t>> regions;
  for (Slot& sl : c->slots) {
    for (int i = 0; i < Slot::N_STAGE; i++) if (sl.d_stage[i]) regions.emplace_back(sl.d_stage[i], sl.d_stage_cap[i]);
    regions.emplace_back(sl.d_state, c->max_batch * 24 * 4);
    regions.emplace_back(sl.d_d01, c->max_batch * 3 * GE_WORDS * 4);
    regions.emplace_back(sl.d_buckets, c->max_batch * PREP_BUCKET_SETS * BUCKET_WORDS * 4);
  }
  for (Slot& sl : c->slots) regions.emplace_back(sl.d_trs, std::min<size_t>(4096, c->max_batch) * SMALL_TR_STRIDE);      // the small transcripts (first lanes): a rejected lane's signature (sign-beside-the-check kernels) must not survive the call
  if (c->d_tiny) { regions.emplace_back(c->d_tiny, TINY_OUT); for (size_t i = 0; i < TINY_OUT; i++) nz += c->h_tiny[i] != 0; }      // staged inputs of the tiny calls (device + pinned)
  if (c->d_admit_rng) regions.emplace_back(c->d_admit_rng, c->d_admit_rng_cap);      // the gathered per-lane rng slices of the admission calls
  if (c->d_replay) regions.emplace_back(c->d_replay, c->d_replay_cap);      // the staged nonce_key and the derived nonces of the replay calls
  if (c->d_small) regions.emplace_back(c->d_small, c->d_small_cap);      // the small-batch schedule's partial sums and bucket sets (what single-item calls use)
  for (auto& r : regions) total += r.second;
  if (total > ((size_t)1 << 30)) { c->err = "act_debug_secret_residue: context too large to read back (use a small max_batch)"; return ACT_ERR_ARG; }
  std::vector<uint8_t> buf;
  for (auto& r : regions) {
    buf.resize(r.second);
    HIPCK(c, hipMemcpy(buf.data(), r.first, r.second, hipMemcpyDeviceToHost));
    for (uint8_t b : buf) nz += b != 0;
  }
  *nonzero_bytes = nz;
  return ACT_OK;
}

int act_prof_enable(act_ctx* c, int on) {
  if (!c) return ACT_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  c->prof_on = on != 0;
  if (c->prof_on && !c->prof_base) {
    HIPCK(c, hipSetDevice(c->device));
    HIPCK(c, hipEventCreate(&c->prof_base));
    HIPCK(c, hipEventRecord(c->prof_base, c->slots[0].stream));
    HIPCK(c, hipEventSynchronize(c->prof_base));
  }
  return ACT_OK;
}
int act_prof_reset(act_ctx* c) {
  if (!c) return ACT_ERR_ARG;
  for (int i = 0; i < PK_COUNT; i++) { c->prof_ms[i] = 0; c->prof_launches[i] = 0; c->prof_lanes[i] = 0; c->prof_iv[i].clear(); }
  return ACT_OK;
}
// time during which at least one launch of kernel i was executing (the union of its launch intervals): with two chunks in
// flight on two streams the launches of a kernel overlap, and the sum of their durations exceeds the wall time
int act_prof_get_busy(act_ctx* c, int i, double* ms_busy) {
  if (!c || i < 0 || i >= PK_COUNT || !ms_busy) return ACT_ERR_ARG;
  std::vector<std::pair<float, float>> iv = c->prof_iv[i];
  std::sort(iv.begin(), iv.end());
  double busy = 0; float lo = 0, hi = -1;
  for (auto& v : iv) {
    if (hi < lo || v.first > hi) { if (hi >= lo) busy += hi - lo; lo = v.first; hi = v.second; }
    else if (v.second > hi) hi = v.second;
  }
  if (hi >= lo) busy += hi - lo;
  *ms_busy = busy;
  return ACT_OK;
}
int act_prof_kernel_count(const act_ctx*) { return PK_COUNT; }
const char* act_prof_kernel_name(const act_ctx*, int i) { return (i >= 0 && i < PK_COUNT) ? kProfNames[i] : ""; }
int act_prof_get(act_ctx* c, int i, double* ms_total, uint64_t* launches, uint64_t* lanes) {
  if (!c || i < 0 || i >= PK_COUNT) return ACT_ERR_ARG;
  if (ms_total) *ms_total = c->prof_ms[i];
  if (launches) *launches = c->prof_launches[i];
  if (lanes) *lanes = c->prof_lanes[i];
  return ACT_OK;
}

// measurement knobs (kernels.h): name = the ACT_* variable of rounds 1-5 without the prefix, lower case
int act_tuning_set(const char* name, int64_t value) {
  static const struct { const char* name; TuneKey key; } names[] = {
    {"no_mapped_reads", T_NO_MAPPED_READS}, {"no_stream_probe", T_NO_STREAM_PROBE}, {"no_fused_tiny", T_NO_FUSED_TINY}, {"no_taper", T_NO_TAPER},
    {"no_wide_client", T_NO_WIDE_CLIENT}, {"no_wide_prove", T_NO_WIDE_PROVE}, {"no_wide_sign", T_NO_WIDE_SIGN}, {"no_lds_isolation", T_NO_LDS_ISOLATION},
    {"small_normal_prio", T_SMALL_NORMAL_PRIO}, {"small_trace", T_SMALL_TRACE}, {"small_in_flight", T_SMALL_IN_FLIGHT}, {"small_sub", T_SMALL_SUB},
    {"stagger", T_STAGGER}, {"hard_stagger", T_HARD_STAGGER}, {"host_chunk", T_HOST_CHUNK}, {"cbor_chunk_msgs", T_CBOR_CHUNK_MSGS}, {"ubench_iters", T_UBENCH_ITERS}};
  if (!name) return ACT_ERR_ARG;
  for (const auto& e : names) if (!strcmp(name, e.name)) { g_tune[e.key].store((long)value); return ACT_OK; }
  return ACT_ERR_ARG;
}
