// hipdsp_region_xcorr: the windowed cross-correlation coefficient of many regions (events) of a planar float32 array
// against a list of partner channels over the lags [-L, L] -- per (region, partner) the row of coefficients, the number
// of lags that have one, the position of the largest and the two standard deviations there (the contract is in
// include/hip_dsp.h; the reference has no code for this, its songdetector.py ends on the crosstalk it leaves open).
//
// Two launches on the context's stream, over a work list the host sizes exactly from the region table:
//
//   region_xcorr_kernel    one 256-thread workgroup per (region, partner, chunk).  The chunks of a region are anchored at
//                          the region's OWN start and hold XC_CHUNK = 65536 samples (the last one fewer).  The workgroup
//                          takes its chunk in tiles of XC_TILE = 2048 samples.  Per tile it converts the 2048 samples of
//                          the event window, d = a - K_a, and the 2048 + nl - 1 samples of the partner that the nl valid
//                          lags reach, e = b - K_b, to float64 ONCE (HdChunk, rowpass.h: 16-byte loads whatever the
//                          row's alignment) and keeps them in LDS; a sample that is not finite is staged as NaN.  Only
//                          the valid lags lo ... lo + nl - 1 are staged and computed: nothing outside [0, frames) of a
//                          row is read, and L = 0 does not pay for 1024.
//                          A thread owns XC_RL = 9 consecutive lags and one of nseg segments of the tile and walks the
//                          segment in steps of XC_RT = 8 samples: 8 LDS reads of d (a broadcast: the lanes of a segment
//                          read one address) and 16 of e feed 72 fma for C = sum d e, 72 for B2 = sum e e and 72
//                          additions for B1 = sum e, all float64 in 27 accumulators.  B1 and B2 are FULL sums per lag
//                          (no running differences over the lags): a lag's three sums see exactly the samples of its own
//                          window, in ascending order.  Lane l reads e at l * 9 + const doubles: 18 dwords apart, so
//                          the 32 lanes of a ds_read_b64 group fall on the 32 distinct even bank pairs of the 64 banks
//                          -- no padding needed; that is why a thread owns 9 lags and not 8.  nseg is the largest power
//                          of two with nseg * ceil(W / 9) <= 256 whose partial sums fit into the 48 KB that L = 1024 stages (128
//                          segments of 16 samples at L = 0, 8 of 256 at L = 96, 1 at L = 1024): it depends on max_lag
//                          alone, and a few lags keep all 256 threads busy.
//                          The segments of a lag are added in ascending order through LDS (over the staged tile, which
//                          is no longer needed), the tiles of a chunk in ascending order into the item's partial row in
//                          the scratch (every entry has one owner thread, which keeps it in a register instead while
//                          the row has at most 256 entries -- the same additions), A1 = sum d and A2 = sum d d
//                          likewise: thread t adds d[8t ... 8t+7], the wave a shuffle tree, the four waves in a fixed
//                          order.  All global loads of a tile are issued before the first is used.
//   region_xcorr_finish    one workgroup per (region, partner): adds the chunks' partial rows in ascending order, forms
//                          r per lag, the clamp, the NaN pattern, the float32 rounding, and reduces count and first
//                          largest value in a fixed order (wave shuffles, then the four waves through LDS).
//
// A non-finite sample cannot be lost from a float64 sum once it is a NaN: A1 (B1 of a lag) of a tile is NaN exactly when
// the event window (that lag's partner window) holds one in that tile.  The partial row stores that as a flag for the
// event window and as a NaN B1 per lag, and the finish reads nothing else of a flagged row or lag.
// No atomics at all.  Index arithmetic on the array is 64-bit.
#include "rowpass.h"
#include <vector>

namespace {

constexpr int XC_THREADS = 256;
typedef HdChunk<XC_THREADS, 2> XcLoad;                  // 2048 samples: two 16-byte loads per thread
constexpr int XC_TILE = XcLoad::CHUNK;                  // samples staged in LDS at a time
constexpr int XC_CHUNK = 32 * XC_TILE;                  // samples per work item
constexpr int XC_RL = 9, XC_RT = 8;                     // lags x samples of a thread's register tile
constexpr int XC_MAX_LAG = 1024;
constexpr int XC_LDS_MAX = 2 * XC_TILE + (2 * XC_MAX_LAG + XC_RL) / XC_RL * XC_RL + 2 * XC_RT;    // doubles staged at L = 1024
constexpr int XC_HEAD = 4;                              // doubles in front of a partial row: A1, A2, flag, unused

struct XcRegion {                                       // one row of the uploaded table; row n_regions: ibase = all items
    long long channel, start, n, ibase;
    long long lo, nl;                                   // the valid lags are lo ... lo + nl - 1
};

struct XcShape {                                        // what follows from max_lag alone
    int L, W, WP, nseg, row;                            // WP: W rounded up to whole threads' lags; row: doubles per item
    size_t lds;
};

inline XcShape xc_shape(int L)
{
    XcShape s;
    s.L = L;
    s.W = 2 * L + 1;
    const int nlb = (s.W + XC_RL - 1) / XC_RL;
    s.WP = nlb * XC_RL;
    s.row = XC_HEAD + 3 * s.WP;
    const size_t stage = (size_t)XC_TILE + (size_t)(XC_TILE + s.WP + 2 * XC_RT);
    s.nseg = XC_THREADS;                                // every thread a unit, within the LDS the longest lag takes anyway
    while (s.nseg > 1 && (s.nseg * nlb > XC_THREADS || s.nseg * 3 * s.WP > XC_LDS_MAX)) s.nseg >>= 1;
    const size_t red = (size_t)s.nseg * 3 * (size_t)s.WP;
    s.lds = sizeof(double) * (stage > red ? stage : red);
    return s;
}

__device__ __forceinline__ bool xc_finite(float v) { return (__float_as_uint(v) & 0x7fffffffu) < 0x7f800000u; }

__device__ __forceinline__ double xc_shift(float v, double K)
{
    return xc_finite(v) ? (double)v - K : __longlong_as_double(0x7ff8000000000000LL);
}

// a thread's samples of one XcLoad: fetched for the event window and the partner's before any is used, so that a tile
// waits for memory once
struct XcRegs {
    float4 v[2];
    float hx, tx;
};

__device__ __forceinline__ void xc_fetch(const XcLoad &s, int t, XcRegs &r) { s.load(t, 0.0f, r.v, r.hx, r.tx); }

// ... to dst[0 ... len), shifted
__device__ __forceinline__ void xc_store(double *dst, const XcLoad &s, int t, double K, const XcRegs &r)
{
    if (t < s.head) dst[t] = xc_shift(r.hx, K);
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int i = u * XC_THREADS + t;
        if (i < s.nvec) {
            double *q = dst + s.head + 4 * i;
            q[0] = xc_shift(r.v[u].x, K);
            q[1] = xc_shift(r.v[u].y, K);
            q[2] = xc_shift(r.v[u].z, K);
            q[3] = xc_shift(r.v[u].w, K);
        }
    }
    if (t < s.tail) dst[s.head + 4 * s.nvec + t] = xc_shift(r.tx, K);
}

__global__ __launch_bounds__(XC_THREADS) void region_xcorr_kernel(const float *__restrict__ x, long long pitch,
                                                                  const XcRegion *__restrict__ tab, int n_regions,
                                                                  const int *__restrict__ partners, int WP, int nseg,
                                                                  double *__restrict__ part)
{
    extern __shared__ double xc_lds[];                  // d[XC_TILE] | e[XC_TILE + WP + 16], later red[nseg][3][WP]
    __shared__ double sh_s1[4], sh_s2[4];
    const int t = threadIdx.x;
    const long long g = blockIdx.x;
    double *d = xc_lds, *e = xc_lds + XC_TILE, *red = xc_lds;
    const int ecap = XC_TILE + WP + 2 * XC_RT;

    const XcRegion reg = tab[hd_owner(tab, &XcRegion::ibase, n_regions, g)];
    const long long nch = (reg.n + XC_CHUNK - 1) / XC_CHUNK;
    const long long rel = g - reg.ibase;
    const long long pi = rel / nch, j = rel - pi * nch;
    const float *rowa = x + reg.channel * pitch, *rowb = x + (long long)partners[pi] * pitch;
    // the pivots; one that is not finite shifts nothing (its window is flagged, the other lags keep finite sums)
    const float Kaf = rowa[reg.start], Kbf = rowb[reg.start];
    const double Ka = xc_finite(Kaf) ? (double)Kaf : 0.0, Kb = xc_finite(Kbf) ? (double)Kbf : 0.0;
    const long long c0 = reg.start + j * XC_CHUNK;
    const long long cleft = reg.n - j * XC_CHUNK;
    const int clen = cleft < XC_CHUNK ? (int)cleft : XC_CHUNK;
    const int nl = (int)reg.nl;
    const int nlb = (nl + XC_RL - 1) / XC_RL, units = nlb * nseg, seg = XC_TILE / nseg;
    const int lb = t % nlb, sg = t / nlb, m0 = lb * XC_RL;
    double *prow = part + g * (long long)(XC_HEAD + 3 * WP);
    double A1 = 0.0, A2 = 0.0, run = 0.0;
    bool abad = false;
    const bool keep = 3 * nl <= XC_THREADS;

    for (int at = 0; at < clen; at += XC_TILE) {
        const int len = clen - at < XC_TILE ? clen - at : XC_TILE;
        const int elen = len + nl - 1;                  // <= XC_TILE + 2 * XC_MAX_LAG: two loads
        const long long s0 = c0 + at, b0 = s0 + reg.lo;
        const bool two = elen > XC_TILE;
        const XcLoad la(rowa, s0, s0 + len, 0), lb0(rowb, b0, b0 + elen, 0), lb1(rowb, b0, b0 + elen, two ? 1 : 0);
        XcRegs ra, rb0, rb1;
        xc_fetch(la, t, ra);
        xc_fetch(lb0, t, rb0);
        if (two) xc_fetch(lb1, t, rb1);
        xc_store(d, la, t, Ka, ra);
        for (int i = len + t; i < XC_TILE; i += XC_THREADS) d[i] = 0.0;
        xc_store(e, lb0, t, Kb, rb0);
        if (two) xc_store(e + XC_TILE, lb1, t, Kb, rb1);
        for (int i = elen + t; i < ecap; i += XC_THREADS) e[i] = 0.0;
        __syncthreads();

        // the moments of the event window: positions, not loads, decide who adds what
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const double v = d[8 * t + k];
            s1 += v;
            s2 = fma(v, v, s2);
        }
        for (int w = 32; w >= 1; w >>= 1) {
            s1 += __shfl_down(s1, w, 64);
            s2 += __shfl_down(s2, w, 64);
        }
        if ((t & 63) == 0) {
            sh_s1[t >> 6] = s1;
            sh_s2[t >> 6] = s2;
        }

        double aC[XC_RL], aB1[XC_RL], aB2[XC_RL];
#pragma unroll
        for (int r = 0; r < XC_RL; r++) aC[r] = aB1[r] = aB2[r] = 0.0;
        if (t < units) {
            const int i1 = (sg + 1) * seg < len ? (sg + 1) * seg : len;
            const double *ep = e + m0;
            int i = sg * seg;
            for (; i + XC_RT <= i1; i += XC_RT) {
                double dv[XC_RT], ev[XC_RT + XC_RL - 1];
#pragma unroll
                for (int k = 0; k < XC_RT; k++) dv[k] = d[i + k];
#pragma unroll
                for (int k = 0; k < XC_RT + XC_RL - 1; k++) ev[k] = ep[i + k];
#pragma unroll
                for (int k = 0; k < XC_RT; k++) {
#pragma unroll
                    for (int r = 0; r < XC_RL; r++) {
                        const double ee = ev[k + r];
                        aC[r] = fma(dv[k], ee, aC[r]);
                        aB1[r] += ee;
                        aB2[r] = fma(ee, ee, aB2[r]);
                    }
                }
            }
            for (; i < i1; i++) {                       // the ragged end of the tile, the same operations in the same order
                const double dd = d[i];
#pragma unroll
                for (int r = 0; r < XC_RL; r++) {
                    const double ee = ep[i + r];
                    aC[r] = fma(dd, ee, aC[r]);
                    aB1[r] += ee;
                    aB2[r] = fma(ee, ee, aB2[r]);
                }
            }
        }
        __syncthreads();                                // everybody is done with d and e: red lies over them
        hd_moments_block(sh_s1, sh_s2, s1, s2);
        if (s1 != s1) abad = true;
        A1 += s1;
        A2 += s2;
        if (t < units) {
#pragma unroll
            for (int r = 0; r < XC_RL; r++) {
                red[(sg * 3 + 0) * WP + m0 + r] = aB1[r];
                red[(sg * 3 + 1) * WP + m0 + r] = aB2[r];
                red[(sg * 3 + 2) * WP + m0 + r] = aC[r];
            }
        }
        __syncthreads();
        for (int idx = t; idx < 3 * nl; idx += XC_THREADS) {            // an entry of the partial row has one owner thread
            const int q = idx / nl, m = idx - q * nl;
            double s = red[q * WP + m];
            for (int k = 1; k < nseg; k++) s += red[(k * 3 + q) * WP + m];
            if (keep) {                                 // ... which holds it in a register while the row has at most 256
                run = at == 0 ? s : run + s;
            } else {
                double *o = prow + XC_HEAD + q * WP + m;
                *o = at == 0 ? s : *o + s;
            }
        }
        __syncthreads();                                // red is read before the next tile is staged over it
    }
    if (keep && t < 3 * nl) prow[XC_HEAD + (t / nl) * WP + t % nl] = run;
    if (t == 0) {
        prow[0] = A1;
        prow[1] = A2;
        prow[2] = abad ? 1.0 : 0.0;
        prow[3] = 0.0;
    }
}

// (value, position) pairs: the larger value wins, equal values keep the earlier position; -1 = no candidate
__device__ __forceinline__ void xc_higher(float &v, int &i, double &sd, float ov, int oi, double osd)
{
    if (oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i))) {
        v = ov;
        i = oi;
        sd = osd;
    }
}

__global__ __launch_bounds__(XC_THREADS) void region_xcorr_finish(const XcRegion *__restrict__ tab, int n_partners, int L,
                                                                  int WP, const double *__restrict__ part,
                                                                  float *__restrict__ out, long long out_pitch,
                                                                  double *__restrict__ info)
{
    __shared__ float sh_v[4];
    __shared__ int sh_i[4], sh_c[4];
    __shared__ double sh_sd[4];
    const int t = threadIdx.x;
    const long long rp = blockIdx.x;
    const long long r = rp / n_partners, pi = rp - r * n_partners;
    const XcRegion reg = tab[r];
    const long long nch = (reg.n + XC_CHUNK - 1) / XC_CHUNK;
    const long long row = XC_HEAD + 3 * WP;
    const double *p0 = part + (reg.ibase + pi * nch) * row;
    float *orow = out + rp * out_pitch;
    const int W = 2 * L + 1;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const float nanf = __uint_as_float(0x7fc00000u);

    double A1 = 0.0, A2 = 0.0;
    bool abad = false;
    for (long long j = 0; j < nch; j++) {               // every thread the same sums in the same order
        A1 += p0[j * row];
        A2 += p0[j * row + 1];
        abad = abad || p0[j * row + 2] != 0.0;
    }
    const double n = (double)reg.n;
    const double ma = A1 / n;
    double va = A2 / n - ma * ma;
    if (!(va > 0.0)) va = 0.0;
    const double sda = sqrt(va);

    float bv = 0.0f;
    int bi = -1, count = 0;
    double bsd = nan;
    for (int pos = t; pos < W; pos += XC_THREADS) {     // ascending positions: a later equal value does not replace
        const long long m = (long long)(pos - L) - reg.lo;
        float v = nanf;
        double sdb = nan;
        if (reg.n > 0 && !abad && m >= 0 && m < reg.nl) {
            double B1 = 0.0, B2 = 0.0, C = 0.0;
            for (long long j = 0; j < nch; j++) {
                const double *q = p0 + j * row + XC_HEAD + m;
                B1 += q[0];
                B2 += q[WP];
                C += q[2 * WP];
            }
            if (B1 == B1) {                             // no sample of this lag's partner window was NaN or +-inf
                const double mb = B1 / n;
                double vb = B2 / n - mb * mb;
                if (!(vb > 0.0)) vb = 0.0;
                sdb = sqrt(vb);
                if (va > 0.0 && vb > 0.0) {
                    double rr = (C / n - ma * mb) / (sda * sdb);
                    rr = rr > 1.0 ? 1.0 : rr < -1.0 ? -1.0 : rr;
                    v = (float)rr;
                }
            }
        }
        orow[pos] = v;
        if (v == v) {
            count++;
            xc_higher(bv, bi, bsd, v, pos, sdb);
        }
    }
    for (int w = 32; w >= 1; w >>= 1) {
        const float ov = __shfl_down(bv, w, 64);
        const int oi = __shfl_down(bi, w, 64);
        const double osd = __shfl_down(bsd, w, 64);
        xc_higher(bv, bi, bsd, ov, oi, osd);
        count += __shfl_down(count, w, 64);
    }
    if ((t & 63) == 0) {
        sh_v[t >> 6] = bv;
        sh_i[t >> 6] = bi;
        sh_sd[t >> 6] = bsd;
        sh_c[t >> 6] = count;
    }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < 4; w++) {
            xc_higher(bv, bi, bsd, sh_v[w], sh_i[w], sh_sd[w]);
            count += sh_c[w];
        }
        double *o = info + rp * 4;
        o[0] = (double)count;
        o[1] = (double)bi;
        o[2] = reg.n > 0 && !abad ? sda : nan;
        o[3] = bi >= 0 ? bsd : nan;
    }
}

}  // namespace

extern "C" int hipdsp_region_xcorr(hipdsp_ctx *ctx, const float *x, int64_t x_pitch, int64_t channels, int64_t frames,
                                   const int64_t *host_regions, int64_t n_regions, const int *host_partners, int n_partners,
                                   int max_lag, float *out, int64_t out_pitch, double *info)
{
    HD_REQUIRE(ctx != nullptr, "ctx is NULL");
    HD_REQUIRE(max_lag >= 0, "max_lag %d is negative", max_lag);
    if (max_lag > XC_MAX_LAG) {
        hipdsp_set_error("max_lag %d: at most %d lags to either side per call", max_lag, XC_MAX_LAG);
        return HIPDSP_ERR_UNSUPPORTED;
    }
    HD_REQUIRE(n_partners >= 0, "negative size");
    HD_TRY(hd_check_table("hipdsp_region_xcorr", ctx, x, x_pitch, channels, frames, host_regions, n_regions, 1LL << 31));
    const XcShape sh = xc_shape(max_lag);
    if (out_pitch == 0) out_pitch = sh.W;
    HD_REQUIRE(out_pitch >= sh.W, "out_pitch smaller than 2 max_lag + 1");
    if (n_regions == 0 || n_partners == 0) return HIPDSP_OK;
    HD_REQUIRE(host_partners != nullptr, "NULL partner list");
    HD_REQUIRE(out != nullptr && info != nullptr, "NULL output");
    HD_REQUIRE(((uintptr_t)out & 3) == 0 && ((uintptr_t)info & 7) == 0, "misaligned pointer");
    for (int p = 0; p < n_partners; p++)
        HD_REQUIRE(host_partners[p] >= 0 && host_partners[p] < channels, "partner %d: channel %d not in [0, %lld)", p,
                   host_partners[p], (long long)channels);
    HD_REQUIRE(n_regions * (long long)n_partners <= 0x7fffffffLL, "too many (region, partner) pairs for one call");

    // the table and the partner list travel as one block: XcRegion[n_regions + 1] | int[n_partners]
    const size_t tab_bytes = sizeof(XcRegion) * ((size_t)n_regions + 1);
    std::vector<char> blob(tab_bytes + sizeof(int) * (size_t)n_partners);
    XcRegion *tab = (XcRegion *)blob.data();
    long long items = 0;
    for (int64_t r = 0; r < n_regions; r++) {
        const long long a = host_regions[3 * r + 1], b = host_regions[3 * r + 2], n = b - a;
        const long long lo = -a > -(long long)max_lag ? -a : -(long long)max_lag;
        const long long hi = frames - b < max_lag ? frames - b : max_lag;
        tab[r] = XcRegion{host_regions[3 * r], a, n, items, lo, n > 0 ? hi - lo + 1 : 0};
        items += (long long)n_partners * ((n + XC_CHUNK - 1) / XC_CHUNK);
        HD_REQUIRE(items <= 0x7fffffffLL, "too many work items for one call");
    }
    tab[n_regions] = XcRegion{0, 0, 0, items, 0, 0};
    memcpy(blob.data() + tab_bytes, host_partners, sizeof(int) * (size_t)n_partners);
    HD_REQUIRE(x != nullptr || items == 0, "NULL data pointer");
    HD_CHECK_HIP(hipSetDevice(ctx->device));
    HdCarve carve(nullptr);
    carve.take<char>(blob.size());
    carve.take<double>((size_t)items * (size_t)sh.row);
    void *work = nullptr;
    HD_TRY(hipdsp_scratch(ctx, carve.bytes(), &work));
    HdCarve lay(work);
    const XcRegion *dtab = (const XcRegion *)lay.take<char>(blob.size());
    double *part = lay.take<double>((size_t)items * (size_t)sh.row);
    const int *dpartners = (const int *)((const char *)dtab + tab_bytes);
    HD_TRY(hd_upload_table(ctx, work, blob.data(), blob.size()));
    if (items > 0) {
        if (sh.lds > 48 * 1024)
            HD_CHECK_HIP(hipFuncSetAttribute((const void *)region_xcorr_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)sh.lds));
        hipLaunchKernelGGL(region_xcorr_kernel, dim3((unsigned)items), dim3(XC_THREADS), sh.lds, ctx->stream, x,
                           (long long)x_pitch, dtab, (int)n_regions, dpartners, sh.WP, sh.nseg, part);
        HD_TRY(hd_launch_status("region_xcorr_kernel"));
    }
    hipLaunchKernelGGL(region_xcorr_finish, dim3((unsigned)(n_regions * n_partners)), dim3(XC_THREADS), 0, ctx->stream, dtab,
                       n_partners, max_lag, sh.WP, (const double *)part, out, (long long)out_pitch, info);
    return hd_launch_status("region_xcorr_finish");
}
