// raw() of the CRC-32 tile kernel (pylinac_amd/csrc/zip_kernels.h, compiled in here with png.hip), two ways, in a sustained loop:
//   slice-by-4   the product: pl_crc32 as it is (four 256-entry tables in LDS, 4 KiB a block, four lookups per dword)
//   table-free   the same tile walk with no table: four message bits a step, the register being linear in each of its bits
//                (four masked constants and a shift: about 22 VALU operations per byte)
// over `ranges` ranges of `kib` KiB each (16-byte aligned, whole tiles), both checked against a bit-serial CRC on the host.
//   crc32_variants [ranges=128] [kib=512] [launches=50]
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -Wno-unused-value scripts/ubench/crc32_variants.hip \
//         -o scripts/ubench/crc32_variants
#include "../../pylinac_amd/csrc/png.hip"

#include <cstdio>
#include <cstdlib>
#include <vector>

void pl_set_error(const char*, ...) {}
int pl_check_launch(const char*) { return hipGetLastError() == hipSuccess ? 0 : 3; }
int pl_cu_count() { return 256; }

namespace {

constexpr unsigned nibble_constant(int j) {                 // the register with only bit j set, four steps on
  unsigned v = 1u << j;
  for (int i = 0; i < 4; ++i) v = zp_step(v);
  return v;
}
constexpr unsigned kN0 = nibble_constant(0), kN1 = nibble_constant(1), kN2 = nibble_constant(2), kN3 = nibble_constant(3);

__device__ __forceinline__ unsigned word_table_free(unsigned crc, unsigned w) {
  crc ^= w;
#pragma unroll
  for (int i = 0; i < 8; ++i)
    crc = (crc >> 4) ^ ((0u - (crc & 1u)) & kN0) ^ ((0u - ((crc >> 1) & 1u)) & kN1) ^ ((0u - ((crc >> 2) & 1u)) & kN2) ^
          ((0u - ((crc >> 3) & 1u)) & kN3);
  return crc;
}

// whole tiles of ranges that start on 16-byte boundaries: the product kernel's layout, walk and tail, raw() without a table
__global__ void __launch_bounds__(kZpThreads)
crc_tile_table_free_kernel(const unsigned char* __restrict__ bytes, const int64_t* __restrict__ r_off,
                           const int64_t* __restrict__ r_len, int64_t max_tiles, unsigned* __restrict__ slots) {
  __shared__ unsigned s_tile[16 * kZpRowStride];
  __shared__ unsigned s_part[kZpThreads / PL_WAVE];
  const int64_t r = blockIdx.x, k = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & (PL_WAVE - 1);
  const int64_t len = r_len[r];
  if (k * kZpTile >= len) return;
  const uint4* src = reinterpret_cast<const uint4*>(bytes + r_off[r] + k * kZpTile);
  for (int p = tid; p < kZpTile / 16; p += kZpThreads) {
    const uint4 q = src[p];
    const int col = (4 * p) >> 4, row = (4 * p) & 15;
    s_tile[row * kZpRowStride + col] = q.x, s_tile[(row + 1) * kZpRowStride + col] = q.y;
    s_tile[(row + 2) * kZpRowStride + col] = q.z, s_tile[(row + 3) * kZpRowStride + col] = q.w;
  }
  __syncthreads();
  unsigned crc = 0;
#pragma unroll
  for (int j = 0; j < kZpOwn / 4; ++j) crc = word_table_free(crc, s_tile[j * kZpRowStride + tid]);
  crc = zp_mul(crc, kZp.after[kZpThreads - 1 - tid]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) crc ^= (unsigned)__shfl_xor((int)crc, o, 64);
  if (lane == 0) s_part[tid / PL_WAVE] = crc;
  __syncthreads();
  if (tid < PL_WAVE) {
    unsigned v = 0;
    for (int w = 0; w < kZpThreads / PL_WAVE; ++w) v ^= s_part[w];
    const unsigned f = zp_xpow8_wave(len - (k + 1) * kZpTile, lane);
    if (tid == 0) slots[r * max_tiles + k] = zp_mul(v, f);
  }
}

unsigned host_crc(const unsigned char* p, size_t n) {
  unsigned c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int b = 0; b < 8; ++b) c = zp_step(c);
  }
  return ~c;
}

}  // namespace

int main(int argc, char** argv) {
  const int64_t n = argc > 1 ? atoll(argv[1]) : 128, len = (argc > 2 ? atoll(argv[2]) : 512) * 1024;
  const int launches = argc > 3 ? atoi(argv[3]) : 50;
  if (n < 1 || len < kZpTile || len % kZpTile) return 2;
  const int64_t total = n * len, max_tiles = len / kZpTile;
  std::vector<unsigned char> host((size_t)total);
  unsigned s = 2463534242u;
  for (auto& b : host) {
    s ^= s << 13, s ^= s >> 17, s ^= s << 5;
    b = (unsigned char)(s >> 11);
  }
  std::vector<int64_t> off((size_t)n), lens((size_t)n, len);
  for (int64_t i = 0; i < n; ++i) off[i] = i * len;
  unsigned char *d_bytes, *d_work;
  int64_t *d_off, *d_len;
  uint32_t* d_crc;
  int32_t* d_status;
  const int64_t work = pl_crc32_work_bytes(n, len);
  if (hipMalloc(&d_bytes, total) != hipSuccess || hipMalloc(&d_work, work) != hipSuccess || hipMalloc(&d_off, n * 8) != hipSuccess ||
      hipMalloc(&d_len, n * 8) != hipSuccess || hipMalloc(&d_crc, n * 4) != hipSuccess || hipMalloc(&d_status, n * 4) != hipSuccess)
    return 3;
  hipMemcpy(d_bytes, host.data(), total, hipMemcpyHostToDevice);
  hipMemcpy(d_off, off.data(), n * 8, hipMemcpyHostToDevice);
  hipMemcpy(d_len, lens.data(), n * 8, hipMemcpyHostToDevice);
  hipMemset(d_status, 0, n * 4);
  std::vector<unsigned> want((size_t)n);
  for (int64_t i = 0; i < n; ++i) want[i] = host_crc(host.data() + off[i], (size_t)len);
  auto slice4 = [&]() { return pl_crc32(d_bytes, total, d_off, d_len, n, len, d_crc, d_status, d_work, nullptr); };
  auto table_free = [&]() {
    hipLaunchKernelGGL(crc_tile_table_free_kernel, dim3((unsigned)n, (unsigned)max_tiles), dim3(kZpThreads), 0, nullptr, d_bytes, d_off, d_len,
                       max_tiles, reinterpret_cast<unsigned*>(d_work));
    hipLaunchKernelGGL(zp_crc_fold_kernel, dim3((unsigned)n), dim3(PL_WAVE), 0, nullptr, total, d_off, d_len, len, max_tiles,
                       reinterpret_cast<const unsigned*>(d_work), (const uint32_t*)nullptr, d_crc, d_status);
    return pl_check_launch("table-free");
  };
  hipEvent_t e0, e1;
  hipEventCreate(&e0), hipEventCreate(&e1);
  int bad = 0;
  auto timed = [&](const char* name, auto call) {
    std::vector<unsigned> got((size_t)n);
    hipMemset(d_crc, 0, n * 4);
    if (call() != 0) bad = 1;
    hipDeviceSynchronize();
    hipMemcpy(got.data(), d_crc, n * 4, hipMemcpyDeviceToHost);
    const bool same = got == want;
    if (!same) bad = 1;
    for (int rep = 0; rep < 3; ++rep) {                     // alternated by the caller; each a loop of `launches` calls
      hipEventRecord(e0, nullptr);
      for (int i = 0; i < launches; ++i) call();
      hipEventRecord(e1, nullptr);
      hipEventSynchronize(e1);
      float ms = 0;
      hipEventElapsedTime(&ms, e0, e1);
      printf("%-11s rep %d: %.4f ms per call, %.1f GB/s, equal to the host's CRC: %s\n", name, rep, ms / launches,
             total / (ms / launches * 1e-3) / 1e9, same ? "yes" : "NO");
    }
  };
  printf("%lld ranges of %lld KiB, %d calls per loop\n", (long long)n, (long long)(len / 1024), launches);
  timed("slice-by-4", slice4);
  timed("table-free", table_free);
  timed("slice-by-4", slice4);
  timed("table-free", table_free);
  return bad;
}
