// workspace_impl.inc — included by engine.hip inside its anonymous namespace: the fixed-base tables shared between the contexts of one
// device, and the allocation of a context's two workspace slots.
// ---- fixed-base tables shared between the contexts of one device --------------------------------------------------
// A table is a pure function of (base, window width): contexts with the same Params on the same GPU (the entries of a node
// handle that list a device twice, a verifier context beside a prover context) use one copy.  At 24-bit windows that is
// 23.6 GB and 0.9 s of construction per base saved for every context after the first.  Reference counted; the last context
// to go frees it.  One lock per device, held across construction, so contexts on different GPUs build concurrently and a
// second context on the same GPU waits for the first's table instead of building its own.
struct SharedTable { uint8_t enc[32]; int bits; uint32_t* p; int refs; };
struct DeviceTables { std::mutex mu; std::vector<SharedTable> tabs; };
DeviceTables g_tables[64];

// returns the table (building it on `s` from the decoded base at d_ext if no context of this device has it yet); nullptr =
// the allocation failed (the caller falls back to a narrower width)
uint32_t* table_acquire(int device, const uint8_t enc[32], int bits, const uint32_t* d_ext, hipStream_t s, bool* built) {
  DeviceTables& dt = g_tables[device & 63];
  std::lock_guard<std::mutex> lk(dt.mu);
  for (SharedTable& t : dt.tabs)
    if (t.bits == bits && memcmp(t.enc, enc, 32) == 0) { t.refs++; if (built) *built = false; return t.p; }
  uint32_t* p = nullptr;
  if (hipMalloc(&p, fb_table_words((uint32_t)bits) * 4) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  launch_build_table(d_ext, p, (uint32_t)bits, s);
  if (hipStreamSynchronize(s) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(p); return nullptr; }
  SharedTable t{}; memcpy(t.enc, enc, 32); t.bits = bits; t.p = p; t.refs = 1;
  dt.tabs.push_back(t);
  if (built) *built = true;
  return p;
}
void table_release(int device, uint32_t* p) {
  if (!p) return;
  DeviceTables& dt = g_tables[device & 63];
  std::lock_guard<std::mutex> lk(dt.mu);
  for (size_t i = 0; i < dt.tabs.size(); i++)
    if (dt.tabs[i].p == p) {
      if (--dt.tabs[i].refs == 0) { (void)hipFree(p); dt.tabs.erase(dt.tabs.begin() + i); }
      return;
    }
}
bool table_cached(int device, const uint8_t enc[32], int bits) {
  DeviceTables& dt = g_tables[device & 63];
  std::lock_guard<std::mutex> lk(dt.mu);
  for (SharedTable& t : dt.tabs) if (t.bits == bits && memcmp(t.enc, enc, 32) == 0) return true;
  return false;
}

int workspace_alloc(act_ctx* c) {
  const SpendTranscript st{c->L, 1};      // the slot holds a bound call's stride (DESIGN 4.12); an unbound call keeps its own stride and length inside it
  size_t B = c->max_batch;
  HIPCK(c, hipMalloc(&c->d_group_ctr, GROUP_CTR_WORDS * 4));
  HIPCK(c, hipMemset(c->d_group_ctr, 0, GROUP_CTR_WORDS * 4));
  HIPCK(c, hipMalloc(&c->d_tiny_tr, TINY_MAX * SMALL_TR_STRIDE));
  HIPCK(c, hipDeviceSynchronize());
  { int can = 0; c->wait_value = hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, c->device) == hipSuccess && can; (void)hipGetLastError(); }
  for (Slot& sl : c->slots) {
    HIPCK(c, hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking));
    if (c->wait_value && hipExtMallocWithFlags((void**)&sl.bits_sig, 8, hipMallocSignalMemory) != hipSuccess) {
      (void)hipGetLastError(); sl.bits_sig = nullptr;      // spend_stage1 falls back to events
    }
    HIPCK(c, hipMalloc(&sl.d_tr, B * st.stride()));
    HIPCK(c, hipMalloc(&sl.d_coords, B * (size_t)c->L * NIELS_WORDS * 4));
    HIPCK(c, hipMalloc(&sl.d_d01, B * 3 * GE_WORDS * 4));
    HIPCK(c, hipMalloc(&sl.d_buckets, B * (size_t)std::max(c->L, PREP_BUCKET_SETS) * BUCKET_WORDS * 4));   // >= 3 bucket sets per proof for the per-proof kernels
    HIPCK(c, hipMalloc(&sl.d_xa, B * GE_WORDS * 4));
    HIPCK(c, hipMalloc(&sl.d_flags, B * 4));
    HIPCK(c, hipMalloc(&sl.d_xof, B * 64));
    HIPCK(c, hipMalloc(&sl.d_status, B));
    HIPCK(c, hipMalloc(&sl.d_trs, B * SMALL_TR_STRIDE));
    HIPCK(c, hipMalloc(&sl.d_state, B * 24 * 4));
    HIPCK(c, hipMalloc(&sl.d_slot, B * 4));
    HIPCK(c, hipMalloc(&sl.d_naf, B * NAF_WORDS * 4));
    HIPCK(c, hipMalloc(&sl.d_dig, B * (size_t)c->L * 8 * 4));
    HIPCK(c, hipMemsetAsync(sl.d_trs, 0, B * SMALL_TR_STRIDE, sl.stream));
    // the secret-bearing buffers start clean (the allocator may hand back another context's freed memory) and are
    // returned to that state by every call (finish_call)
    HIPCK(c, hipMemsetAsync(sl.d_state, 0, B * 24 * 4, sl.stream));
    HIPCK(c, hipMemsetAsync(sl.d_d01, 0, B * 3 * GE_WORDS * 4, sl.stream));
    HIPCK(c, hipMemsetAsync(sl.d_buckets, 0, B * PREP_BUCKET_SETS * BUCKET_WORDS * 4, sl.stream));
  }
  return ACT_OK;
}
