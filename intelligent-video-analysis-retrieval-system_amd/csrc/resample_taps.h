// The tap tables of Pillow's 8-bit resampler (Resample.c precompute_coeffs + normalize_coeffs_8bpc), built on the host: shared by
// the frame preprocessing (bicubic / bilinear, preprocess.hip) and the perceptual hash (Lanczos, phash.hip).
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

namespace ivr_resample {

constexpr int kPrecisionBits = 32 - 8 - 2;

enum Filter { kBicubic = 0, kBilinear = 1, kLanczos = 2 };

struct Taps {          // one resampling axis, for the surviving output positions only
    int out_len = 0;   // positions computed
    int ksize = 0;
    int in_lo = 0, in_hi = 0;   // union of input positions touched
    std::vector<int32_t> xmin, xcnt, kk;   // kk is [ksize][out_len] (tap-major: coalesced across positions)
};

inline double filt_bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}
inline double filt_bilinear(double x) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}
inline double filt_sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return std::sin(x) / x;
}
inline double filt_lanczos(double x) {       // truncated sinc on [-3, 3)
    if (-3.0 <= x && x < 3.0) return filt_sinc(x) * filt_sinc(x / 3);
    return 0.0;
}

// output positions [first, first+count) of a full-axis resize in_size -> out_size
inline Taps make_taps(int in_size, int out_size, int first, int count, Filter filter) {
    Taps t;
    double (*fn)(double) = filter == kBilinear ? filt_bilinear : (filter == kLanczos ? filt_lanczos : filt_bicubic);
    const double fsupport = filter == kBilinear ? 1.0 : (filter == kLanczos ? 3.0 : 2.0);
    const double scale = (double)in_size / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = fsupport * filterscale;
    t.ksize = (int)std::ceil(support) * 2 + 1;
    t.out_len = count;
    t.xmin.resize(count);
    t.xcnt.resize(count);
    t.kk.assign((size_t)t.ksize * count, 0);
    t.in_lo = in_size;
    t.in_hi = 0;
    const double ss = 1.0 / filterscale;
    std::vector<double> k(t.ksize);
    for (int i = 0; i < count; ++i) {
        const int xx = first + i;
        const double center = (xx + 0.5) * scale;
        int lo = (int)(center - support + 0.5);
        if (lo < 0) lo = 0;
        int hi = (int)(center + support + 0.5);
        if (hi > in_size) hi = in_size;
        const int n = hi - lo;
        double ww = 0.0;
        for (int x = 0; x < n; ++x) {
            const double w = fn((x + lo - center + 0.5) * ss);
            k[x] = w;
            ww += w;
        }
        for (int x = 0; x < n; ++x) {
            if (ww != 0.0) k[x] /= ww;
            const double v = k[x] * (1 << kPrecisionBits);
            t.kk[(size_t)x * count + i] = k[x] < 0 ? (int)(-0.5 + v) : (int)(0.5 + v);
        }
        t.xmin[i] = lo;
        t.xcnt[i] = n;
        if (lo < t.in_lo) t.in_lo = lo;
        if (hi > t.in_hi) t.in_hi = hi;
    }
    return t;
}

}  // namespace ivr_resample
