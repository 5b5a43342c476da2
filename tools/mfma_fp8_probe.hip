// mfma_fp8_probe: one v_mfma_f32_16x16x32_fp8_fp8 per case on operands read from a file, the 16 x 16 results written to
// another: how does the instruction add its 32 products?  (Not in fp32: see tests/fp8_emulation.py, mfma_fp8_dot.)
// Input file: int32 ncase; A e4m3 bytes [ncase][16 rows][32 k]; B e4m3 bytes [ncase][16 cols][32 k]; C float
// [ncase][16][16].  Output: D float [ncase][16][16] = A B^T + C.  tools/mfma_fp8_probe.py writes the cases, runs this
// and compares the results with candidate accumulation rules.
//   hipcc -O2 --offload-arch=gfx950 tools/mfma_fp8_probe.hip -o tools/mfma_fp8_probe.bin
//   python tools/mfma_fp8_probe.py
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ void probe(const unsigned char* A, const unsigned char* B, const float* C, float* D, int ncase) {
    const int lane = threadIdx.x & 63, g = lane >> 4, r = lane & 15;
    for (int cs = blockIdx.x; cs < ncase; cs += gridDim.x) {
        long a = *reinterpret_cast<const long*>(A + ((long)cs * 16 + r) * 32 + 8 * g);
        long b = *reinterpret_cast<const long*>(B + ((long)cs * 16 + r) * 32 + 8 * g);
        f32x4 c;
        for (int i = 0; i < 4; ++i) c[i] = C[((long)cs * 16 + 4 * g + i) * 16 + r];
        c = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, b, c, 0, 0, 0);
        for (int i = 0; i < 4; ++i) D[((long)cs * 16 + 4 * g + i) * 16 + r] = c[i];
    }
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s cases.in results.out\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror("in"); return 1; }
    int ncase = 0;
    if (fread(&ncase, 4, 1, f) != 1 || ncase <= 0 || ncase > 100000) return 1;
    std::vector<unsigned char> A((size_t)ncase * 512), B((size_t)ncase * 512);
    std::vector<float> C((size_t)ncase * 256), D((size_t)ncase * 256);
    if (fread(A.data(), 1, A.size(), f) != A.size()) return 1;
    if (fread(B.data(), 1, B.size(), f) != B.size()) return 1;
    if (fread(C.data(), 4, C.size(), f) != C.size()) return 1;
    fclose(f);
    unsigned char *dA, *dB; float *dC, *dD;
    CK(hipMalloc(&dA, A.size())); CK(hipMalloc(&dB, B.size())); CK(hipMalloc(&dC, C.size() * 4)); CK(hipMalloc(&dD, D.size() * 4));
    CK(hipMemcpy(dA, A.data(), A.size(), hipMemcpyHostToDevice));
    CK(hipMemcpy(dB, B.data(), B.size(), hipMemcpyHostToDevice));
    CK(hipMemcpy(dC, C.data(), C.size() * 4, hipMemcpyHostToDevice));
    probe<<<dim3(ncase < 1024 ? ncase : 1024), dim3(64)>>>(dA, dB, dC, dD, ncase);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(D.data(), dD, D.size() * 4, hipMemcpyDeviceToHost));
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror("out"); return 1; }
    fwrite(D.data(), 4, D.size(), o);
    fclose(o);
    printf("ok %d cases\n", ncase);
    return 0;
}
