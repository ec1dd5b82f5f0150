// LDS-array cost of the instruction forms of the fp64 element trips at N = 5 (degree 4), on the kernel's own address
// patterns: cycles of a CU per wave instruction, 16 waves per CU (4 per SIMD, as the block kernel), fixed trip counts,
// no wave waits for another.  Lane 25 s + 5 b + c works on element slot s of its wave (slots of 130 entries, lanes 50-63
// masked off), as kernels.hpp elem_compute:
//   own   (a, b, c)   entries s 130 + a 25 + b 5 + c    a = 0..3
//   idx1  (b, k, c)   entries s 130 + b 25 + k 5 + c    k = 0..3
//   idx2  (b, c, k)   entries s 130 + b 25 + c 5 + k    k = 0..3
//   bcast             the 21 map coefficients of the lane's element: every lane of an element reads one address
// Forms: ds_read_b64 x 4 against ds_read2_b64 x 2, ds_write_b64 x 4 against ds_write2_b64 x 2, 20 broadcast reads as
// ds_read_b64 x 20 / ds_read2_b64 x 10 / ds_read_b128 x 10 (cell stride 22: 16-byte aligned), ds_add_f64 on distinct
// and on colliding addresses.  The instructions are written out (inline assembly with its own waits) so that each row
// times the form it names.  Each wave stamps s_memtime around its loop; s_memrealtime (100 MHz) gives the clock.
//   hipcc --offload-arch=gfx950 -O2 tools/lds_probe.hip -o tools/_bin/lds_probe
// Run the built program through tools/gpu_lds_probe.sh only: it gives it a time limit of its own and keeps the table.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <vector>

typedef double d2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) double lds_double;

enum { OWN = 0, IDX1 = 1, IDX2 = 2, BCAST = 3, ADD = 4 };
enum { RD1 = 0, RD2 = 1, WR1 = 2, WR2 = 3, RD128 = 4, ADD1 = 5, ADD2 = 6, ADD8 = 7, ADDK = 8 };

constexpr int LDS_ENTRIES = 5120;   // 40 KB per block: exactly four blocks of four waves per CU

#define LDS_WAIT() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

// one group: four 8-byte accesses of the pattern (STEP entries apart), in the named form
template <int FORM, int STEP>
__device__ __forceinline__ void group(unsigned addr, double& acc)
{
  if constexpr (FORM == RD1)
  {
    double v0, v1, v2, v3;
    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=&v"(v0) : "v"(addr), "n"(0 * STEP * 8));
    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=&v"(v1) : "v"(addr), "n"(1 * STEP * 8));
    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=&v"(v2) : "v"(addr), "n"(2 * STEP * 8));
    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=&v"(v3) : "v"(addr), "n"(3 * STEP * 8));
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3)::"memory");   // the sums wait for the data
    acc += (v0 + v1) + (v2 + v3);
  }
  else if constexpr (FORM == RD2)
  {
    d2 v0, v1;
    asm volatile("ds_read2_b64 %0, %1 offset0:%2 offset1:%3" : "=&v"(v0) : "v"(addr), "n"(0 * STEP), "n"(1 * STEP));
    asm volatile("ds_read2_b64 %0, %1 offset0:%2 offset1:%3" : "=&v"(v1) : "v"(addr), "n"(2 * STEP), "n"(3 * STEP));
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v0), "+v"(v1)::"memory");
    acc += (v0.x + v0.y) + (v1.x + v1.y);
  }
  else if constexpr (FORM == WR1)
  {
    asm volatile("ds_write_b64 %0, %1 offset:%2" ::"v"(addr), "v"(acc), "n"(0 * STEP * 8) : "memory");
    asm volatile("ds_write_b64 %0, %1 offset:%2" ::"v"(addr), "v"(acc), "n"(1 * STEP * 8) : "memory");
    asm volatile("ds_write_b64 %0, %1 offset:%2" ::"v"(addr), "v"(acc), "n"(2 * STEP * 8) : "memory");
    asm volatile("ds_write_b64 %0, %1 offset:%2" ::"v"(addr), "v"(acc), "n"(3 * STEP * 8) : "memory");
    LDS_WAIT();
  }
  else if constexpr (FORM == WR2)
  {
    asm volatile("ds_write2_b64 %0, %1, %2 offset0:%3 offset1:%4" ::"v"(addr), "v"(acc), "v"(acc), "n"(0 * STEP),
                 "n"(1 * STEP)
                 : "memory");
    asm volatile("ds_write2_b64 %0, %1, %2 offset0:%3 offset1:%4" ::"v"(addr), "v"(acc), "v"(acc), "n"(2 * STEP),
                 "n"(3 * STEP)
                 : "memory");
    LDS_WAIT();
  }
  else if constexpr (FORM == RD128)
  {
    d2 v0, v1;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=&v"(v0) : "v"(addr), "n"(0 * STEP * 8));
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=&v"(v1) : "v"(addr), "n"(2 * STEP * 8));
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v0), "+v"(v1)::"memory");
    acc += (v0.x + v0.y) + (v1.x + v1.y);
  }
  else   // ds_add_f64, four regions of 1 KB
  {
    const double one = 1.0;
    asm volatile("ds_add_f64 %0, %1 offset:0" ::"v"(addr), "v"(one) : "memory");
    asm volatile("ds_add_f64 %0, %1 offset:1024" ::"v"(addr), "v"(one) : "memory");
    asm volatile("ds_add_f64 %0, %1 offset:2048" ::"v"(addr), "v"(one) : "memory");
    asm volatile("ds_add_f64 %0, %1 offset:3072" ::"v"(addr), "v"(one) : "memory");
    LDS_WAIT();
  }
}

template <int PAT, int FORM>
__global__ __launch_bounds__(256) void k_probe(long long* __restrict__ ticks, long long* __restrict__ real,
                                               double* __restrict__ sink, int iters)
{
  __shared__ __attribute__((aligned(16))) double lds[LDS_ENTRIES];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int i = tid; i < LDS_ENTRIES; i += 256)
    lds[i] = 1e-3 * i;
  __syncthreads();
  const int s = lane / 25, r = lane % 25, b = r / 5, c = r % 5;
  // entry of the lane's first access; everything stays below 4 * 260 + 4 * 44 + 512 entries of the 5120
  int e;
  if (PAT == OWN)
    e = w * 260 + s * 130 + b * 5 + c;
  else if (PAT == IDX1)
    e = w * 260 + s * 130 + b * 25 + c;
  else if (PAT == IDX2)
    e = w * 260 + s * 130 + b * 25 + c * 5;
  else if (PAT == BCAST)
    e = 1040 + (2 * w + s) * (FORM == RD128 ? 22 : 21);
  else   // ADD: distinct addresses, 2 or 8 lanes per address, or the kernel's typical column (stride 5 entries)
    e = 2048 + (FORM == ADD1 ? lane : FORM == ADD2 ? (lane >> 1) : FORM == ADD8 ? (lane >> 3) : s * 125 + b * 5 + c);
  const unsigned addr = (unsigned)(size_t)((lds_double*)lds) + 8u * (unsigned)e;
  double acc = 1e-9 * lane;
  const long long r0 = __builtin_amdgcn_s_memrealtime();
  const long long t0 = __builtin_amdgcn_s_memtime();
  if (lane < 50)
  {
    for (int it = 0; it < iters; ++it)
    {
      if constexpr (PAT == BCAST)   // 20 of the 21 coefficients: five groups of four consecutive values
      {
        group<FORM, 1>(addr, acc);
        group<FORM, 1>(addr + 32, acc);
        group<FORM, 1>(addr + 64, acc);
        group<FORM, 1>(addr + 96, acc);
        group<FORM, 1>(addr + 128, acc);
      }
      else
      {
        constexpr int STEP = PAT == OWN ? 25 : PAT == IDX1 ? 5 : 1;
        group<FORM, STEP>(addr, acc);
        group<FORM, STEP>(addr, acc);
        group<FORM, STEP>(addr, acc);
        group<FORM, STEP>(addr, acc);
      }
    }
  }
  const long long t1 = __builtin_amdgcn_s_memtime();
  const long long r1 = __builtin_amdgcn_s_memrealtime();
  if (lane == 0)
  {
    ticks[blockIdx.x * 4 + w] = t1 - t0;
    real[blockIdx.x * 4 + w] = r1 - r0;
  }
  sink[(size_t)blockIdx.x * 256 + tid] = acc;
}

#define CHECK(x)                                                                 \
  do                                                                             \
  {                                                                              \
    hipError_t e_ = (x);                                                         \
    if (e_ != hipSuccess)                                                        \
    {                                                                            \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                    \
      return 1;                                                                  \
    }                                                                            \
  } while (0)

static long long *d_ticks, *d_real;
static double* d_sink;
static int nblocks;

template <int PAT, int FORM>
static int run(const char* pattern, const char* form, int accesses_per_instr)
{
  const int iters = 2000, nw = nblocks * 4;
  const int acc_per_iter = (PAT == BCAST) ? 20 : 16;
  for (int rep = 0; rep < 2; ++rep)   // the first launch warms up
  {
    hipLaunchKernelGGL((k_probe<PAT, FORM>), dim3(nblocks), dim3(256), 0, 0, d_ticks, d_real, d_sink, iters);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
  }
  std::vector<long long> t(nw), r(nw);
  CHECK(hipMemcpy(t.data(), d_ticks, nw * sizeof(long long), hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(r.data(), d_real, nw * sizeof(long long), hipMemcpyDeviceToHost));
  std::sort(t.begin(), t.end());
  std::sort(r.begin(), r.end());
  const double ticks = (double)t[nw / 2], mhz = ticks / ((double)r[nw / 2] / 100.0);
  const double per_access = ticks / ((double)iters * acc_per_iter * 16);   // 16 waves share the CU's LDS
  printf("%-6s %-16s  %7.2f cycles/wave-instruction  %6.2f per 8-byte access   (clock %.0f MHz, wave spread %.1f %%)\n",
         pattern, form, per_access * accesses_per_instr, per_access, mhz,
         100.0 * (double)(t[nw - 1] - t[0]) / ticks);
  return 0;
}

int main()
{
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  nblocks = 4 * prop.multiProcessorCount;
  CHECK(hipMalloc(&d_ticks, sizeof(long long) * nblocks * 4));
  CHECK(hipMalloc(&d_real, sizeof(long long) * nblocks * 4));
  CHECK(hipMalloc(&d_sink, sizeof(double) * nblocks * 256));
  printf("# %s, %d CUs, %d blocks of 4 waves (4 blocks per CU), 50 of 64 lanes active\n", prop.name,
         prop.multiProcessorCount, nblocks);
  int bad = 0;
  bad |= run<OWN, RD1>("own", "ds_read_b64", 1);
  bad |= run<OWN, RD2>("own", "ds_read2_b64", 2);
  bad |= run<IDX1, RD1>("idx1", "ds_read_b64", 1);
  bad |= run<IDX1, RD2>("idx1", "ds_read2_b64", 2);
  bad |= run<IDX2, RD1>("idx2", "ds_read_b64", 1);
  bad |= run<IDX2, RD2>("idx2", "ds_read2_b64", 2);
  bad |= run<BCAST, RD1>("bcast", "ds_read_b64", 1);
  bad |= run<BCAST, RD2>("bcast", "ds_read2_b64", 2);
  bad |= run<BCAST, RD128>("bcast", "ds_read_b128", 2);
  bad |= run<OWN, WR1>("own", "ds_write_b64", 1);
  bad |= run<OWN, WR2>("own", "ds_write2_b64", 2);
  bad |= run<IDX1, WR1>("idx1", "ds_write_b64", 1);
  bad |= run<IDX1, WR2>("idx1", "ds_write2_b64", 2);
  bad |= run<IDX2, WR1>("idx2", "ds_write_b64", 1);
  bad |= run<IDX2, WR2>("idx2", "ds_write2_b64", 2);
  bad |= run<ADD, ADD1>("add", "ds_add_f64 x1", 1);
  bad |= run<ADD, ADD2>("add", "ds_add_f64 x2", 1);
  bad |= run<ADD, ADD8>("add", "ds_add_f64 x8", 1);
  bad |= run<ADD, ADDK>("add", "ds_add_f64 col", 1);
  return bad;
}
