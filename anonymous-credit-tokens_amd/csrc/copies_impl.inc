// copies_impl.inc — included by engine.hip behind admit_impl.inc: the copy stage of act_redeem_(cbor_)admit_unique_batch (DESIGN 4.7;
// kernels in k_copies.hip, lane bodies in copy_lanes.h).  It runs between the screen's compaction and verification, over the m
// survivors in their compact order:
//   a. fingerprint   fp[j] of survivor j's input bytes      device memory: k_copy_fp; host memory: the same lane body on the host workers
//   b. leader table  leader[j] = the smallest j with fp[j]  k_copy_claim / k_copy_leader in both cases (8 bytes per lane go up)
//   c. compare       copy_of[j] = leader[j] iff every byte is equal: k_copy_equal, or the host workers (4 bytes per lane come down)
//   d. mark          pre2 = pre with COPY_MARK on the copies, lead[lane] = a copy's leader lane       k_copy_mark
//   e. compaction    launch_admit_compact over pre2: the lanes that are verified, in lane order
// The caller goes on with v (idx2 / pos2 / pre2 where there are copies, else the screen's arrays as passed) and launches k_copy_resolve behind the scatter -- or, in
// the replay unique forms (act_redeem_(cbor_)admit_replay_unique_batch), k_copy_serve behind both scatters: a copy gets its leader's refund.
// Everything staged here is public (proof bytes never leave the caller's memory; fingerprints and lane numbers are derived from them).
namespace {

struct CopyHostJob { CopySpan span; const uint32_t* idx; const uint32_t* leader; const uint32_t* salt; uint64_t* fp; uint32_t* copy_of; uint32_t m; };

}  // namespace

int AdmitCopies::run(hipStream_t stream, bool dev, size_t n, const CopySpan& span, const uint32_t* h_idx, const uint32_t salt[4]) {
  const uint8_t* const d_pre = v.pre; const uint32_t* const d_idx = v.idx; const size_t m = v.m;      // the screen's survivors, as passed
  copies = 0; m2 = m;
  if (m < 2) return ACT_OK;                                   // nothing to be a copy of
  uint32_t cap = 4; while (cap < 2 * m) cap <<= 1;
  const size_t nb = (n + ADMIT_BLOCK - 1) / ADMIT_BLOCK;
  size_t need = 0;
  auto take = [&](size_t bytes) { const size_t at = need; need += (bytes + 15) & ~(size_t)15; return at; };
  const size_t o_fp = take(m * 8), o_tfp = take((size_t)cap * 8), o_tj = take((size_t)cap * 4), o_slot = take(m * 4), o_leader = take(m * 4), o_copy = take(m * 4);
  const size_t o_pre2 = take(n), o_lead = take(n * 4), o_idx2 = take(n * 4), o_pos2 = take(n * 4), o_blk = take(nb * 4), o_total = take(4);
  int rc = d.alloc(need);
  if (rc) { c->err = "admission: copy stage"; return rc; }
  ADCK(c, hipSetDevice(c->device));
  uint64_t* const d_fp = reinterpret_cast<uint64_t*>(d.p + o_fp);
  uint32_t* const d_leader = reinterpret_cast<uint32_t*>(d.p + o_leader); uint32_t* const d_copy = reinterpret_cast<uint32_t*>(d.p + o_copy);
  d_pre2 = d.p + o_pre2; d_lead = reinterpret_cast<uint32_t*>(d.p + o_lead);
  d_idx2 = reinterpret_cast<uint32_t*>(d.p + o_idx2); d_pos2 = reinterpret_cast<uint32_t*>(d.p + o_pos2);
  ADCK(c, hipMemsetAsync(d.p + o_tfp, 0, (size_t)cap * 8, stream));
  ADCK(c, hipMemsetAsync(d.p + o_tj, 0xFF, (size_t)cap * 4, stream));
  ADCK(c, hipMemsetAsync(d_lead, 0xFF, n * 4, stream));
  ADCK(c, hipMemcpyAsync(d_pre2, d_pre, n, hipMemcpyDeviceToDevice, stream));

  // ---- a. fingerprints -------------------------------------------------------------------------------------------------------------------
  std::vector<uint64_t> h_fp; std::vector<uint32_t> h_leader, h_copy;
  CopyHostJob job{span, h_idx, nullptr, salt, nullptr, nullptr, (uint32_t)m};
  if (dev) {
    CopyFpArgs fa{span, d_idx, (uint32_t)m, {}, d_fp}; memcpy(fa.salt.w, salt, 16);
    launch_copy_fp(fa, stream);
  } else {
    h_fp.assign(m, 0); job.fp = h_fp.data();
    act_host_parallel_for(m, 16, 0, [](void* p, size_t j0, size_t j1) {
      const CopyHostJob& J = *static_cast<const CopyHostJob*>(p);
      for (size_t j = j0; j < j1; j++) {
        const uint32_t lane = J.idx[j]; const uint64_t len = copy_len(J.span, lane); const uint8_t* src = J.span.src + copy_beg(J.span, lane);
        J.fp[j] = copy_fp_finish(copy_fp_sum(src, len, J.salt), len, J.salt);
      }
    }, &job);
    ADCK(c, hipMemcpyAsync(d_fp, h_fp.data(), m * 8, hipMemcpyHostToDevice, stream));
  }
  // ---- b. the leader table ---------------------------------------------------------------------------------------------------------------
  CopyTableArgs ta{d_fp, (uint32_t)m, reinterpret_cast<uint64_t*>(d.p + o_tfp), reinterpret_cast<uint32_t*>(d.p + o_tj), cap, reinterpret_cast<uint32_t*>(d.p + o_slot), d_leader};
  launch_copy_leaders(ta, stream);
  ADCK(c, hipGetLastError());
  // ---- c. the exact compare --------------------------------------------------------------------------------------------------------------
  if (dev) {
    CopyEqualArgs ea{span, d_idx, d_leader, (uint32_t)m, d_copy};
    launch_copy_equal(ea, stream);
  } else {
    h_leader.assign(m, 0); h_copy.assign(m, COPY_NONE);
    ADCK(c, hipMemcpyAsync(h_leader.data(), d_leader, m * 4, hipMemcpyDeviceToHost, stream));
    ADCK(c, hipStreamSynchronize(stream));
    for (size_t j = 0; j < m; j++) if (h_leader[j] > j) { c->err = "admission: the leader table named a later lane"; return ACT_ERR_HIP; }
    job.leader = h_leader.data(); job.copy_of = h_copy.data();
    act_host_parallel_for(m, 16, 0, [](void* p, size_t j0, size_t j1) {
      const CopyHostJob& J = *static_cast<const CopyHostJob*>(p);
      const CopyEqualArgs ea{J.span, J.idx, J.leader, J.m, J.copy_of};
      for (size_t j = j0; j < j1; j++) {
        const uint8_t *x = nullptr, *y = nullptr; uint64_t len = 0;
        bool same = copy_equal_ranges(ea, (uint32_t)j, &x, &y, &len);
        if (same) same = copy_equal_all(x, y, len);
        J.copy_of[j] = same ? J.leader[j] : COPY_NONE;
      }
    }, &job);
    ADCK(c, hipMemcpyAsync(d_copy, h_copy.data(), m * 4, hipMemcpyHostToDevice, stream));
  }
  // ---- d, e. the side array and the second compaction ------------------------------------------------------------------------------------
  CopyMarkArgs ma{d_idx, d_copy, (uint32_t)m, d_pre2, d_lead};
  launch_copy_mark(ma, stream);
  uint32_t m32 = 0;
  launch_admit_compact(d_pre2, (uint32_t)n, reinterpret_cast<uint32_t*>(d.p + o_blk), d_idx2, d_pos2, reinterpret_cast<uint32_t*>(d.p + o_total), stream);
  ADCK(c, hipGetLastError());
  ADCK(c, hipMemcpyAsync(&m32, d.p + o_total, 4, hipMemcpyDeviceToHost, stream));
  ADCK(c, hipStreamSynchronize(stream));
  if (m32 == 0 || m32 > m) { c->err = "admission: the copy stage counted survivors it cannot have"; return ACT_ERR_HIP; }      // (a leader always survives)
  m2 = m32; copies = m - m2;
  if (copies) v = {d_pre2, d_idx2, d_pos2, m2};      // the lanes that are verified: the second compaction's
  return ACT_OK;
}

// Debug / test hook (include/act_mi355x.h): the leader table alone over fingerprints the caller makes up -- forced collisions and the
// single-slot flood on the device, and the time of the two launches
extern "C" int act_debug_copy_leaders(act_ctx* c, size_t m, const uint64_t* fp, uint32_t* out_leader, double* out_ms) {
  if (out_ms) *out_ms = 0;
  if (!c || m > ((size_t)1 << 30) || (m && (!fp || !out_leader))) return ACT_ERR_ARG;
  if (!m) return ACT_OK;
  for (size_t j = 0; j < m; j++) if (!fp[j]) { c->err = "act_debug_copy_leaders: a fingerprint is never 0"; return ACT_ERR_ARG; }
  uint32_t cap = 4; while (cap < 2 * m) cap <<= 1;
  DevTmp d(c);
  const size_t o_tfp = (m * 8 + 15) & ~(size_t)15, o_tj = o_tfp + (size_t)cap * 8, o_slot = o_tj + (size_t)cap * 4, o_leader = o_slot + ((m * 4 + 15) & ~(size_t)15);
  int rc = d.alloc(o_leader + m * 4);
  if (rc) return rc;
  ADCK(c, hipSetDevice(c->device));
  hipStream_t stream = nullptr;
  hipEvent_t e0, e1;
  ADCK(c, hipEventCreate(&e0)); ADCK(c, hipEventCreate(&e1));
  struct Ev { hipEvent_t a, b; ~Ev() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } ev{e0, e1};
  ADCK(c, hipMemcpyAsync(d.p, fp, m * 8, hipMemcpyHostToDevice, stream));
  ADCK(c, hipMemsetAsync(d.p + o_tfp, 0, (size_t)cap * 8, stream));
  ADCK(c, hipMemsetAsync(d.p + o_tj, 0xFF, (size_t)cap * 4, stream));
  CopyTableArgs ta{reinterpret_cast<uint64_t*>(d.p), (uint32_t)m, reinterpret_cast<uint64_t*>(d.p + o_tfp), reinterpret_cast<uint32_t*>(d.p + o_tj), cap,
                   reinterpret_cast<uint32_t*>(d.p + o_slot), reinterpret_cast<uint32_t*>(d.p + o_leader)};
  ADCK(c, hipEventRecord(e0, stream));
  launch_copy_leaders(ta, stream);
  ADCK(c, hipGetLastError());
  ADCK(c, hipEventRecord(e1, stream));
  ADCK(c, hipMemcpyAsync(out_leader, d.p + o_leader, m * 4, hipMemcpyDeviceToHost, stream));
  ADCK(c, hipStreamSynchronize(stream));
  float ms = 0;
  ADCK(c, hipEventElapsedTime(&ms, e0, e1));
  if (out_ms) *out_ms = ms;
  return ACT_OK;
}
