// Accuracy probe of the device math library: tanhf, sinf and cosf as csrc/frame_ops.hip's k_pose_update calls them (built with the
// flags of SRCS_EXACT, see the Makefile here).  Stand-alone: reads a file of raw float32 arguments, evaluates the three functions on
// the device, prints one line per argument -- the bits of the argument and of the three results, in hex.  measure.py feeds it and
// compares with float64; the record is profiles/libm_ulp_gfx950.json.  It does not touch the kernel under test.
//   probe <args.f32>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define CHECK(x)                                                                                  \
  do {                                                                                            \
    hipError_t e_ = (x);                                                                          \
    if (e_ != hipSuccess) {                                                                       \
      std::fprintf(stderr, "%s: %s (%s:%d)\n", #x, hipGetErrorString(e_), __FILE__, __LINE__);    \
      return 1;                                                                                   \
    }                                                                                             \
  } while (0)

__global__ void k_probe(const float* __restrict__ x, float* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float v = x[i];
  out[i] = tanhf(v);
  out[n + i] = sinf(v);
  out[2 * n + i] = cosf(v);
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s <file of raw float32 arguments>\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  std::vector<float> x;
  float buf[4096];
  size_t got;
  while ((got = std::fread(buf, sizeof(float), 4096, f)) > 0) x.insert(x.end(), buf, buf + got);
  std::fclose(f);
  const size_t n = x.size();
  if (n == 0 || n > ((size_t)1 << 26)) {
    std::fprintf(stderr, "need 1 .. 2^26 arguments, got %zu\n", n);
    return 2;
  }
  float *dx = nullptr, *dout = nullptr;
  CHECK(hipMalloc(&dx, n * sizeof(float)));
  CHECK(hipMalloc(&dout, 3 * n * sizeof(float)));
  CHECK(hipMemcpy(dx, x.data(), n * sizeof(float), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_probe, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dx, dout, n);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  std::vector<float> out(3 * n);
  CHECK(hipMemcpy(out.data(), dout, 3 * n * sizeof(float), hipMemcpyDeviceToHost));
  CHECK(hipFree(dx));
  CHECK(hipFree(dout));
  auto bits = [](float v) { uint32_t b; std::memcpy(&b, &v, 4); return b; };
  for (size_t i = 0; i < n; ++i)
    std::printf("%08x %08x %08x %08x\n", bits(x[i]), bits(out[i]), bits(out[n + i]), bits(out[2 * n + i]));
  return 0;
}
