// rate_terms.h -- the per-element rate terms of the eval-mode statistics, shared by the kernels that sum them over images and channels
// (pointwise.hip) and the ones that keep them by position (rate_map.hip): one definition, so every form adds the same fp32 values.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_math.h"

// Eval-mode rate estimate (qarv/model.py:95-96; CompressAI GaussianConditional._likelihood): per latent element
// P = Phi((.5-|v|)/s) - Phi((-.5-|v|)/s), v = zhat - mean = the integer symbol, s = max(exp(softplus(x+2.3)-2.3), bound),
// P = max(P, 1e-9).  Phi in fp32 as the reference: erf form for DiscretizedGaussian (underflows to exactly 0 in the tails), erfc form
// for stock GaussianConditional.
// ln P of one latent element (the per-element arithmetic of every lvae_gaussian_nll_* entry point).
__device__ __forceinline__ float gaussian_logp(float lv, int32_t sym, float bound, int cdf_form) {
    const float xs = lv + 2.3f;
    const float sp = xs > 20.0f ? xs : log1pf(expf(xs));
    const float s = fmaxf(expf(sp - 2.3f), bound);
    const float v = fabsf((float)sym);
    const float a = (0.5f - v) / s, d = (-0.5f - v) / s;
    float up, lo;
    if (cdf_form == 0) {
        up = 0.5f * (1.0f + lvae_erff(a * 0.70710678118654752440f));
        lo = 0.5f * (1.0f + lvae_erff(d * 0.70710678118654752440f));
    } else {
        up = 0.5f * erfcf(-0.70710678118654752440f * a);
        lo = 0.5f * erfcf(-0.70710678118654752440f * d);
    }
    const float P = fmaxf(up - lo, 1e-9f);
    return logf(P);
}

// Lossless model: one term of GaussianNLLOutputNet.forward_loss (qresvae/model.py:24-38, entropy_coding.py:18-49) in fp32 with torch's
// operation order: logscale = softplus(l + 16) - 16 (threshold 20), s = exp(logscale), x = (im - 0.5)*2, bin b = 1/127.5,
// P = Phi((x + b/2 - m)/s) - Phi((x - b/2 - m)/s) with Phi(v) = 0.5*(1 + erf((v - m)*(1/s)/sqrt 2));
// log P = P > 1e-6 ? log(max(P, 1e-8)) : -(x - m)^2/(2 s^2) - log s - log sqrt(2 pi) + log b.  The mean is not rounded (that belongs to
// the coder).  m / l: the out net's mean and raw log-scale of one sample, t: the image value in [0, 1].
// Contraction is off here because it was off where this term came from: pixel_nll_kernel (pointwise.hip) carries the pragma for its whole
// body, so that the expression keeps torch's operation order; the pragma moved with the term and lvae_pixel_nll_f32 keeps its bits.
// gaussian_logp above never had it (its erf does, device_math.h) and does not get it now, for the same reason: lvae_gaussian_nll_f32,
// _map_ and _chan_ keep the bits they had.  The position kernel's equality with the map kernel then rests on both translation units
// compiling this one inlined body alike, which tests/test_gpu_rate_map.py checks bit for bit for both CDF forms.
__device__ __forceinline__ float pixel_logp(float m, float l, float t) {
#pragma clang fp contract(off)
    const float hb = (float)(0.5 * (1.0 / 127.5));
    const float log_bin = (float)-4.848116364598481;                      // math.log(1/127.5)
    const float log_sqrt_2pi = (float)0.9189385332046727;                 // math.log(math.sqrt(2 * math.pi))
    const float sqrt2 = 1.41421356237309504880f;                           // math.sqrt(2), the divisor of torch's Normal.cdf
    float ls = l + 16.0f;
    ls = ls > 20.0f ? ls : log1pf(expf(ls));
    ls = ls - 16.0f;
    const float s = expf(ls);
    const float inv = 1.0f / s;
    const float x = (t - 0.5f) * 2.0f;
    const float up = 0.5f * (1.0f + erff((((x + hb) - m) * inv) / sqrt2));
    const float lo = 0.5f * (1.0f + erff((((x - hb) - m) * inv) / sqrt2));
    const float P = up - lo;
    float lp;
    if (P > 1e-6f) {
        lp = logf(fmaxf(P, 1e-8f));
    } else {
        const float d = x - m;
        lp = -(d * d) / (2.0f * (s * s)) - logf(s) - log_sqrt_2pi;
        lp = lp + log_bin;
    }
    return lp;
}
