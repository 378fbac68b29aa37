// What dynamic-LDS request does a launch get without / with hipFuncAttributeMaxDynamicSharedMemorySize?  A trivial in-bounds
// kernel; a refused launch is a host-side error code, nothing runs.
#include <hip/hip_runtime.h>
#include <cstdio>

__global__ void probe_kernel(float* out, int n) {
  extern __shared__ float sm[];
  for (int i = threadIdx.x; i < n; i += blockDim.x) sm[i] = (float)i;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = sm[n - 1];
}
__global__ void probe_kernel2(float* out, int n) {      // never opted in
  extern __shared__ float sm[];
  for (int i = threadIdx.x; i < n; i += blockDim.x) sm[i] = (float)i;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = sm[n - 1] + 1.f;
}

template <typename F>
static void try_launch(F fn, const char* tag, float* d, size_t bytes) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(fn, dim3(1), dim3(256), bytes, 0, d, (int)(bytes / 4));
  hipError_t e = hipGetLastError();
  hipError_t s = hipDeviceSynchronize();
  float h = -1.f;
  if (e == hipSuccess && s == hipSuccess) (void)hipMemcpy(&h, d, 4, hipMemcpyDeviceToHost);
  printf("%s %6zu B: launch %s, sync %s, last word %.0f (want %zu)\n", tag, bytes, hipGetErrorName(e), hipGetErrorName(s), h,
         bytes / 4 - 1);
}

int main() {
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, 0) != hipSuccess) { printf("no device\n"); return 2; }
  int optin = -1, perblk = -1;
  (void)hipDeviceGetAttribute(&perblk, hipDeviceAttributeMaxSharedMemoryPerBlock, 0);
  (void)hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin, 0);
  printf("%s: sharedMemPerBlock %zu, attr MaxSharedMemoryPerBlock %d, SharedMemPerBlockOptin %d, maxSharedMemoryPerMultiProcessor %zu\n",
         p.gcnArchName, p.sharedMemPerBlock, perblk, optin, p.maxSharedMemoryPerMultiProcessor);
  hipFuncAttributes fa;
  if (hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(probe_kernel)) == hipSuccess)
    printf("before opt-in: maxDynamicSharedSizeBytes %d sharedSizeBytes %zu\n", fa.maxDynamicSharedSizeBytes, fa.sharedSizeBytes);
  float* d = nullptr;
  if (hipMalloc(&d, 64) != hipSuccess) return 3;
  const size_t sizes[] = {40 * 1024, 49152, 49408, 64768, 65280, 65536, 66816, 80640};
  for (size_t b : sizes) try_launch(probe_kernel2, "no opt-in  ", d, b);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(probe_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 80640);
  printf("hipFuncSetAttribute(80640): %s\n", hipGetErrorName(e));
  if (hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(probe_kernel)) == hipSuccess)
    printf("after opt-in: maxDynamicSharedSizeBytes %d\n", fa.maxDynamicSharedSizeBytes);
  for (size_t b : sizes) try_launch(probe_kernel, "opted in   ", d, b);
  (void)hipFree(d);
  return 0;
}
