// The 1024-point dense-DFT machinery that K18 (spectralgate.hip) and K19 (formant.hip) share: the per-device basis / window tables
// and the K-split GEMM helper on the exact-fp32 matrix-core kernel of conv.hip.  The spectrum is TIME-major, S[frame][row], re rows
// [0, 513), im rows [576, 1089); the inverse wants the spectral rows outermost, ST[row][frame].
#pragma once
#include <math.h>

#include <mutex>
#include <vector>

#include "conv.h"

namespace rvc {

constexpr int SG_NFFT = 1024;
constexpr int SG_BINS = 513;
constexpr int SG_IM0 = 576;            // im rows start here (re rows padded 513 -> 576)
constexpr int SG_ROWS = 1152;          // 2 x 576: a multiple of 128 (GEMM columns forward, K inverse)

struct GateTables {
    float *fwd = nullptr;      // [1024][1152]  cos | -sin
    float *inv = nullptr;      // [1152][1024]  w_k cos / 1024 | -w_k sin / 1024, w = 1 for DC and Nyquist, 2 between
    float *window = nullptr;   // [1024] periodic hann
    int device = -1;
};
inline std::mutex g_gate_mutex;
inline std::vector<GateTables> g_gate_tabs;   // one per device that has run a 1024-point transform (common.h: per-device resources)

inline int gate_tables_for_device(GateTables *out) {
    GateTables tab;
    RVC_HIP(hipGetDevice(&tab.device));
    std::lock_guard<std::mutex> lock(g_gate_mutex);
    for (const GateTables &t : g_gate_tabs)
        if (t.device == tab.device) { *out = t; return 0; }
    std::vector<float> fwd((size_t)SG_NFFT * SG_ROWS, 0.f), inv((size_t)SG_ROWS * SG_NFFT, 0.f), window(SG_NFFT);
    for (int n = 0; n < SG_NFFT; ++n)
        for (int k = 0; k < SG_BINS; ++k) {
            const int ph = (int)(((int64_t)k * n) % SG_NFFT);   // exact argument reduction
            const double a = 2.0 * M_PI * (double)ph / SG_NFFT, c = cos(a), s = sin(a);
            const bool edge = k == 0 || k == SG_NFFT / 2;        // real bins of a real signal: counted once, imaginary part ignored
            fwd[(size_t)n * SG_ROWS + k] = (float)c;
            fwd[(size_t)n * SG_ROWS + SG_IM0 + k] = (float)(-s);
            inv[(size_t)k * SG_NFFT + n] = (float)((edge ? 1.0 : 2.0) * c / SG_NFFT);
            inv[(size_t)(SG_IM0 + k) * SG_NFFT + n] = edge ? 0.f : (float)(-2.0 * s / SG_NFFT);
        }
    for (int n = 0; n < SG_NFFT; ++n) window[n] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * n / SG_NFFT));
    auto up = [](const void *h, size_t bytes, void **d) -> hipError_t {
        hipError_t e = hipMalloc(d, bytes);
        if (e == hipSuccess) e = hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice);
        return e;
    };
    hipError_t e = up(fwd.data(), fwd.size() * 4, (void **)&tab.fwd);
    if (e == hipSuccess) e = up(inv.data(), inv.size() * 4, (void **)&tab.inv);
    if (e == hipSuccess) e = up(window.data(), window.size() * 4, (void **)&tab.window);
    if (e != hipSuccess) return fail("1024-point DFT: table upload failed: %s", hipGetErrorString(e));
    g_gate_tabs.push_back(tab);
    *out = tab;
    return 0;
}

// y[m][c] = sum_k W[k][m] X[k][c] for m < m_pad, c < cols, k < K: the frames (forward) or the transposed spectrum (inverse) as the
// conv kernel's "weights", the DFT basis as its "activation".  One launch sums its k range as ONE fmaf chain per output, and a
// chain's rounding grows with its length and with the size of its partial sums -- here the partial sum reaches the full size of
// a tonal bin (forward), or sits at the sample's size from the tone's bin on (inverse).  So K is walked in `splits` launches,
// each chain starting from zero and the epilogue adding the sum so far (accin, which may alias y): the same products as short
// chains plus splits - 1 adds in a fixed order.  The forward transform takes 16 x 64 terms -- its error reaches K18's output
// twice, through S and through the mask, whose sigmoid multiplies the relative error of |S| by up to 2.5 A / M -- the inverse
// 4 x 288.  Measured on K18's 48 kHz test signal at prop_decrease = 1 (max |device - float64| in units of the float32 SciPy
// path's own error): 9.5 unsplit, 14.1 at 4 / 4, 5.5 at 16 / 4; with both transforms exact it would be 1.0 (DESIGN, K18).
constexpr int SG_SPLIT_FWD = 16, SG_SPLIT_INV = 4;
inline int gate_gemm(const float *X, int K, int cols, const float *W, int m_pad, float *y, int splits, hipStream_t stream) {
    const int kb = K / splits;   // 64 forward, 288 inverse: multiples of the kernel's 8-row chunks
    for (int b = 0; b < splits; ++b) {
        ConvParams p;
        p.x1 = X + (size_t)b * kb * cols; p.c1 = kb; p.slope1 = 1.f; p.x1_bstride = (int64_t)kb * cols; p.l_in = cols;
        p.w = W + (size_t)b * kb * m_pad;
        p.accin = b ? y : nullptr;
        p.y = y; p.y_bstride = (int64_t)m_pad * cols; p.m_total = m_pad; p.c_out = m_pad; p.n_cols = cols; p.l_out = cols;
        p.kw = 1; p.dil = 1; p.padl = 0; p.batch = 1;
        if (launch_conv(p, stream)) return 1;
    }
    return 0;
}

}  // namespace rvc
