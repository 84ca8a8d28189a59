// Placement of two-wave workgroups shaped like the two-wave affine flux kernel: 128 threads, 256 VGPRs, 38 kB of LDS.
// Answers: how many workgroups are resident on a CU at once, do the two waves of a workgroup sit on different SIMDs, and
// does every SIMD carry two waves?  Records HW_ID / XCC_ID of every wave and the wall-clock interval of every workgroup.
// build: hipcc -O2 --offload-arch=gfx950 tools/probes/two_wave_probe.hip -o two_wave_probe ; run it on an MI355X.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#include <map>
#include <algorithm>

__global__ __launch_bounds__(128) void probe(unsigned *out, long long *when, int spin)
{
  __shared__ double big[4750]; // 38.0 kB
  const int w = threadIdx.x >> 6;
  unsigned hw, xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  asm volatile("v_mov_b32 v255, 0" ::: "v255"); // the allocation of the flux kernel: 256 VGPRs, two waves per SIMD
  big[threadIdx.x] = hw;
  big[4749 - threadIdx.x] = xcc;
  __syncthreads();
  const long long t0 = wall_clock64();
  double acc = big[(threadIdx.x * 7) % 128];
  for (int i = 0; i < spin; i++) acc = acc * 1.0000001 + 1e-9;
  const long long t1 = wall_clock64();
  if ((threadIdx.x & 63) == 0)
  {
    out[(blockIdx.x * 2 + w) * 2 + 0] = hw;
    out[(blockIdx.x * 2 + w) * 2 + 1] = xcc;
    when[(blockIdx.x * 2 + w) * 2 + 0] = t0;
    when[(blockIdx.x * 2 + w) * 2 + 1] = t1;
  }
  if (acc == 12345.678) out[0] = 0;
}

int main()
{
  const int nwg = 2048;
  unsigned *d;
  long long *dw;
  if (hipMalloc(&d, sizeof(unsigned) * nwg * 4) != hipSuccess || hipMalloc(&dw, sizeof(long long) * nwg * 4) != hipSuccess) return 1;
  int occ = 0;
  (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, probe, 128, 0);
  printf("occupancy query: %d workgroups per CU\n", occ);
  hipLaunchKernelGGL(probe, dim3(nwg), dim3(128), 0, 0, d, dw, 200000);
  if (hipDeviceSynchronize() != hipSuccess) return 1;
  std::vector<unsigned> h(nwg * 4);
  std::vector<long long> t(nwg * 4);
  hipMemcpy(h.data(), d, sizeof(unsigned) * h.size(), hipMemcpyDeviceToHost);
  hipMemcpy(t.data(), dw, sizeof(long long) * t.size(), hipMemcpyDeviceToHost);
  // gfx9 HW_ID: wave_id[3:0] simd_id[5:4] pipe_id[7:6] cu_id[11:8] sh_id[12] se_id[15:13]
  auto simd = [&](int b, int w) { return (h[(b * 2 + w) * 2] >> 4) & 3; };
  std::map<unsigned, std::vector<int>> by_cu;
  for (int b = 0; b < nwg; b++)
  {
    const unsigned hw = h[(b * 2) * 2], xcc = h[(b * 2) * 2 + 1] & 0xf;
    by_cu[(xcc << 12) | (((hw >> 13) & 7) << 8) | (((hw >> 12) & 1) << 4) | ((hw >> 8) & 0xf)].push_back(b);
  }
  printf("distinct CUs seen: %zu\n", by_cu.size());
  long split = 0, resident_hist[16] = {}, even = 0, sets = 0, simd_load_hist[16] = {};
  for (int b = 0; b < nwg; b++) split += simd(b, 0) != simd(b, 1);
  int shown = 0;
  for (auto &kv : by_cu)
  {
    // the workgroups that were running when the CU's first one ended: the first resident set
    std::vector<int> &v = kv.second;
    long long first_end = t[(v[0] * 2) * 2 + 1];
    for (int b : v) first_end = std::min(first_end, t[(b * 2) * 2 + 1]);
    int n = 0, load[4] = {0, 0, 0, 0};
    for (int b : v)
      if (t[(b * 2) * 2] < first_end)
      {
        n++;
        load[simd(b, 0)]++;
        load[simd(b, 1)]++;
      }
    resident_hist[std::min(n, 15)]++;
    sets++;
    even += load[0] == 2 && load[1] == 2 && load[2] == 2 && load[3] == 2;
    for (int s = 0; s < 4; s++) simd_load_hist[std::min(load[s], 15)]++;
    if (shown++ < 6)
    {
      printf("CU key %05x: resident %d:", kv.first, n);
      for (int b : v)
        if (t[(b * 2) * 2] < first_end) printf("  wg %d [simd%u/slot%u simd%u/slot%u]", b, simd(b, 0), h[(b * 2) * 2] & 0xf, simd(b, 1), h[(b * 2 + 1) * 2] & 0xf);
      printf("\n");
    }
  }
  printf("workgroups whose two waves sit on different SIMDs: %ld of %d\n", split, nwg);
  printf("workgroups resident at once per CU (count of CUs):");
  for (int i = 0; i < 16; i++)
    if (resident_hist[i]) printf("  %d: %ld", i, resident_hist[i]);
  printf("\nCUs whose first resident set puts two waves on every SIMD: %ld of %ld\n", even, sets);
  printf("waves per SIMD in the first resident set (count of SIMDs):");
  for (int i = 0; i < 16; i++)
    if (simd_load_hist[i]) printf("  %d: %ld", i, simd_load_hist[i]);
  printf("\n");
  return 0;
}
