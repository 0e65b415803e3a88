// The stamp dump of the measurement build GVI_FUSED_TIMING (tools/build_variant.py): what factor_fused_kernel's waves and
// blocks wrote into the stamp buffer of launch_fused_t, read back and reported on stderr.  Included by launch_factor.inc under
// that macro only, inside its anonymous namespace; the product build never sees this file.
//
//   holds      fused_timing_dump: the read-back and the four reports -- [walk stamps] per wave and item, [prep stamps] of block
//              0, [fused stamps] of eight blocks with their hardware ids, [cu stamps] / [cu summary] of every item block by CU
//   relies on  host_ctx.inc (gvi_ctx); kernels_fused.hpp (FusedArgs, FUSED_BLOCK_STAMPS and the stamp layout)
//   defines    no entry point
//
// The caller (launch_fused_t) owns the buffer, the GVI_FUSED_DBG bits and the count of launches that decides WHEN to dump.

// stamps: [1120] wave stamps of the first blocks, then [FUSED_BLOCK_STAMPS][5] per item block; 100 MHz ticks
void fused_timing_dump(gvi_ctx* c, const FusedArgs& A, const unsigned long long* stamps) {
  unsigned long long h[1120];
  (void)hipStreamSynchronize(c->stream);
  (void)hipMemcpy(h, stamps, sizeof(h), hipMemcpyDeviceToHost);
  for (int blk = 0; blk < 8; ++blk)
    for (int w = 0; w < 4; ++w)
      for (int it = 0; it < 2; ++it) {
        const unsigned long long* ws = h + 352 + ((blk * 4 + w) * 2 + it) * 12;
        fprintf(stderr, "[walk stamps] block %4d wave %d item %d: shader cycles prologue %llu | s=1 %llu (%llu tiles) | s=2 %llu (%llu) | s=3 %llu (%llu) | s=4 %llu (%llu) | reduction %llu\n",
                blk * 146, w, it, ws[0], ws[1], ws[7], ws[2], ws[8], ws[3], ws[9], ws[4], ws[10], ws[5]);
      }
  for (int w = 0; w < 4; ++w) {
    fprintf(stderr, "[prep stamps] block 0 wave %d, us after the wave's start: prologue [arguments warm | first scalars | barrier] %.2f %.2f %.2f; gather [entry | loads back | stores issued] %.2f %.2f %.2f; products [Sigma row loaded | Cholesky | L^-1 | LDS | Lam + stores | H, u0]:",
            w, (double)(long long)(h[256 + 16 * w + 11] - h[8 * w]) * 0.01, (double)(long long)(h[256 + 16 * w + 12] - h[8 * w]) * 0.01,
            (double)(long long)(h[256 + 16 * w + 13] - h[8 * w]) * 0.01, (double)(long long)(h[256 + 16 * w + 8] - h[8 * w]) * 0.01, (double)(long long)(h[256 + 16 * w + 9] - h[8 * w]) * 0.01, (double)(long long)(h[256 + 16 * w + 10] - h[8 * w]) * 0.01);
    for (int i = 0; i < 6; ++i) fprintf(stderr, " %.2f", (double)(long long)(h[256 + 16 * w + i] - h[8 * w]) * 0.01);
    fprintf(stderr, "\n");
  }
  unsigned long long t0 = ~0ull;
  for (int blk = 0; blk < 8; ++blk) if (h[blk * 32] && h[blk * 32] < t0) t0 = h[blk * 32];
  for (int blk = 0; blk < 8; ++blk)
    for (int w = 0; w < 4; ++w) {
      const unsigned hw = (unsigned)h[320 + blk * 4 + w], xcc = (unsigned)(h[320 + blk * 4 + w] >> 32);
      fprintf(stderr, "[fused stamps] block %4d wave %d (xcc %u se %u cu %2u simd %u slot %2u; absolute, us after the first start):", blk * 146, w,
              xcc & 15, (hw >> 13) & 7, (hw >> 8) & 15, (hw >> 4) & 3, hw & 15);
      for (int i = 0; i < 8; ++i) fprintf(stderr, " %.2f", h[blk * 32 + w * 8 + i] ? (double)(long long)(h[blk * 32 + w * 8 + i] - t0) * 0.01 : -1.0);
      fprintf(stderr, "\n");
    }
  // every item block, grouped by CU: the residency slots of one CU against each other
  std::vector<unsigned long long> hb(5 * (size_t)FUSED_BLOCK_STAMPS);
  (void)hipMemcpy(hb.data(), stamps + 1120, hb.size() * 8, hipMemcpyDeviceToHost);
  struct Blk { int b; double start, p2, bar, end; unsigned slot; };
  std::map<unsigned, std::vector<Blk>> cus;                 // (xcc, se, cu) -> its blocks
  unsigned long long tb0 = ~0ull;
  for (int b = 0; b < A.nblk && b < FUSED_BLOCK_STAMPS; ++b) if (hb[(size_t)b * 5] && hb[(size_t)b * 5] < tb0) tb0 = hb[(size_t)b * 5];
  for (int b = 0; b < A.nblk && b < FUSED_BLOCK_STAMPS; ++b) {
    const unsigned long long* q = hb.data() + (size_t)b * 5;
    if (!q[0] || !q[2]) continue;
    const unsigned hw = (unsigned)q[3], xcc = (unsigned)(q[3] >> 32) & 15;
    auto us = [&](unsigned long long t) { return (double)(long long)(t - tb0) * 0.01; };
    cus[(xcc << 8) | ((hw >> 8) & 255)].push_back({b, us(q[0]), us(q[1]), us(q[2]), us(q[4]), hw & 15});   // (HW_ID bits 15:8: se_id, sh_id, cu_id)
  }
  std::vector<double> spread_bar, spread_end, first_bar, last_bar, walk_first, walk_last;
  int shown = 0;
  for (auto& [id, v] : cus) {
    std::sort(v.begin(), v.end(), [](const Blk& a, const Blk& b) { return a.bar < b.bar; });
    double e0 = 1e300, e1 = -1e300;
    for (const Blk& x : v) { e0 = std::min(e0, x.end); e1 = std::max(e1, x.end); }
    if (v.size() == 4) {
      spread_bar.push_back(v.back().bar - v.front().bar); spread_end.push_back(e1 - e0);
      first_bar.push_back(v.front().bar); last_bar.push_back(v.back().bar);
      walk_first.push_back(v.front().bar - v.front().start); walk_last.push_back(v.back().bar - v.back().start);
    }
    if (shown++ < 6)
      for (const Blk& x : v)
        fprintf(stderr, "[cu stamps] xcc %u se %u cu %2u: block %4d slot %2u, us after the first walk start: walk start %.2f, wave 0 ends phase 2 %.2f, "
                "behind the barrier %.2f, last exit %.2f\n", id >> 8, (id >> 5) & 7, id & 31, x.b, x.slot, x.start, x.p2, x.bar, x.end);
  }
  auto stat = [](std::vector<double> v, double* med, double* mx) {
    std::sort(v.begin(), v.end());
    *med = v.empty() ? 0.0 : v[v.size() / 2]; *mx = v.empty() ? 0.0 : v.back();
  };
  double m[6], x[6];
  stat(spread_bar, &m[0], &x[0]); stat(spread_end, &m[1], &x[1]); stat(first_bar, &m[2], &x[2]); stat(last_bar, &m[3], &x[3]);
  stat(walk_first, &m[4], &x[4]); stat(walk_last, &m[5], &x[5]);
  fprintf(stderr, "[cu summary] walk_prio %d, %zu CUs with four stamped blocks (of %zu): end of phase 2 (behind the barrier), first-to-last block of a CU: "
          "median %.2f max %.2f us; first block at median %.2f, last at median %.2f max %.2f us; walk (start to barrier) of the first block median %.2f, "
          "of the last median %.2f max %.2f us; last exit, first-to-last: median %.2f max %.2f us\n", A.walk_prio, spread_bar.size(), cus.size(),
          m[0], x[0], m[2], m[3], x[3], m[4], m[5], x[5], m[1], x[1]);
}
