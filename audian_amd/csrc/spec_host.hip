// spec_host.hip -- the host-side rules that hipdsp_spectrogram (spectrogram.hip), the fused sweeps (chain.hip) and the
// event spectra (regionspectra.hip) share: how many frames lie inside a trace, the window's sum of squares behind the
// PSD scale, and the twiddle / window tables of the FFT kernels.  No device code: one definition each, so the entry
// points that must agree to the bit cannot drift apart (declarations in common.h; tests/test_shim_sanitizers.py runs
// this unit on the CPU under the sanitizers).
#include <cmath>
#include "common.h"

long long hd_frames_valid(long long frames_out, long long avail, int nfft, int hop)
{
    long long nsource = (frames_out - 1) * (long long)hop + nfft;
    if (nsource > avail) nsource = avail;
    long long n_valid = 0;
    if (frames_out > 0 && nsource >= nfft) n_valid = (nsource - (nfft - hop)) / hop;
    if (n_valid > frames_out) n_valid = frames_out;
    return n_valid;
}

double hd_hann_sumsq(int nfft)
{
    double wss = 0.0;
    for (int i = 0; i < nfft; i++) {
        const double w = 0.5 - 0.5 * cos(2.0 * M_PI * (double)i / (double)nfft);
        wss += w * w;
    }
    return wss;
}

namespace {

inline float *put_cis(float *p, double a)
{
    *p++ = (float)cos(a); *p++ = (float)sin(a);
    return p;
}

// the sections in the order the kernels keep them in LDS, computed in float64
void fill_tables(float *p, int nfft, int R1, int R2, int R3)
{
    const int M = nfft / 2;
    for (int t = 1; t < R2; t++)                           // tw2: over R1 * R2 in front of a third stage, over M without
        for (int k = 0; k < R1; k++) p = put_cis(p, -2.0 * M_PI * (double)(k * t) / (double)(R3 > 0 ? R1 * R2 : M));
    if (R3 > 0)
        for (int k = 0; k < R1 * R2; k++) p = put_cis(p, -2.0 * M_PI * (double)k / (double)M);                 // tw3
    for (int k = 0; k <= M / 2; k++) p = put_cis(p, -2.0 * M_PI * (double)k / (double)nfft);                  // twn
    for (int i = 0; i < nfft; i++) *p++ = (float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)i / (double)nfft));    // window
}

}  // namespace

int hd_fft_table_set(hipdsp_ctx *ctx, int nfft, int R1, int R2, int R3, const float **dev)
{
    int lg = 0;
    while ((1 << lg) < nfft) lg++;
    void *&slot = R3 > 0 ? ctx->fft_tables[lg] : ctx->fft_tables2[lg];
    if (!slot) {
        if (hd_capturing(ctx)) {
            hipdsp_set_error("first spectrogram call for nfft %d during stream capture; run it once before", nfft);
            return HIPDSP_ERR_INVALID;
        }
        const int M = nfft / 2;
        const size_t n = 2 * (size_t)((R2 - 1) * R1 + (R3 > 0 ? R1 * R2 : 0) + M / 2 + 1 + M);
        float *h = new float[n];
        fill_tables(h, nfft, R1, R2, R3);
        void *d = nullptr;
        hipError_t e = hipMalloc(&d, n * sizeof(float));
        if (e == hipSuccess) e = hipMemcpy(d, h, n * sizeof(float), hipMemcpyHostToDevice);
        delete[] h;
        if (e != hipSuccess) {
            if (d) (void)hipFree(d);
            HD_CHECK_HIP(e);
        }
        slot = d;
    }
    *dev = (const float *)slot;
    return HIPDSP_OK;
}

int hd_fft_tables(hipdsp_ctx *ctx, int nfft, const float **dev)
{
    if (nfft == 2048) return hd_fft_table_set(ctx, 2048, 16, 16, 4, dev);
    if (nfft == 1024) return hd_fft_table_set(ctx, 1024, 8, 8, 8, dev);
    if (nfft == 512) return hd_fft_table_set(ctx, 512, 8, 8, 4, dev);
    if (nfft == 256) return hd_fft_table_set(ctx, 256, 8, 4, 4, dev);
    hipdsp_set_error("no three-stage table set for nfft %d", nfft);
    return HIPDSP_ERR_UNSUPPORTED;
}
