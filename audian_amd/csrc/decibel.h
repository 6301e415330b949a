// The decibel arithmetic of libhip_dsp, shared by the element-wise kernels (elementwise.hip) and the dB epilogue of
// hipdsp_band_power (bandpower.hip), so that dB there is bit for bit decibel(linear):
//   out = 10*log10(v/ref_power), -inf where v <= min_power        (include/hip_dsp.h; ref_power, min_power are doubles)
// The threshold is compared exactly: the host hands over the largest float not above min_power ((float)min_power may
// round UP -- 1e-7, 0.1, 1e-10 do -- and a power equal to that float is above min_power).  The quotient is the float
// product v * (float)(1/ref_power) wherever that product is a normal float (two roundings of the logarithm's argument,
// none at ref_power == 1); where it is not -- a ref_power whose reciprocal or product leaves float32's normal range, a
// denormal power, +inf, NaN -- the element takes the quotient in float64 (decibel_wide), which any positive finite
// double ref_power can have.
#pragma once
#include <cfloat>
#include <cmath>

struct DbArgs {
    float inv_ref;       // (float)(1/ref_power); 0 where that is no normal float: every element goes the float64 way
    float threshold;     // the largest float <= min_power: v <= threshold in float32 is exactly v <= min_power
    double ref_power;
};

inline DbArgs db_args(double ref_power, double min_power)
{
    DbArgs a;
    a.ref_power = ref_power;
    a.inv_ref = (float)(1.0 / ref_power);
    if (!(a.inv_ref >= FLT_MIN)) a.inv_ref = 0.0f;      // a denormal reciprocal has lost bits (+inf stays: its products are inf or NaN)
    a.threshold = (float)min_power;
    if ((double)a.threshold > min_power) a.threshold = nextafterf(a.threshold, -INFINITY);
    return a;
}

static __device__ __attribute__((noinline)) float decibel_wide(float v, double ref_power)
{
    if (!(v > 0.0f && v <= FLT_MAX)) return 10.0f * log10f(v);       // +inf, NaN; with min_power < 0 also zero and negative powers
    const double r = (double)v / ref_power;
    if (r >= DBL_MIN && r <= DBL_MAX) return (float)(10.0 * log10(r));
    int ev, er;                                                       // the quotient leaves float64 too: mantissas and exponents apart
    const double mv = frexp((double)v, &ev), mr = frexp(ref_power, &er);
    return (float)(10.0 * (log10(mv / mr) + (double)(ev - er) * 0.30102999566398120));
}

__device__ __forceinline__ float decibel_of(float v, const DbArgs &a)
{
    if (v <= a.threshold) return -INFINITY;
    const float q = v * a.inv_ref;
    return (q >= FLT_MIN && q <= FLT_MAX) ? 10.0f * log10f(q) : decibel_wide(v, a.ref_power);
}
