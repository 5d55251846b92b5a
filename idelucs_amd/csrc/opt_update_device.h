// opt_update_device.h -- torch's SGD, Adam and RMSprop-with-momentum updates of one element, and the coefficients a step's update takes, for
// the last launch of a training step: opt_step.hip (NetLinear) and the small_wgrad_opt kernels of small_step.hip (myNet).  One definition:
// both steps are held to torch.optim's results to 1e-5 of a tensor's largest magnitude, and a fix made here reaches both.
//
// Hyperparameters are a DEVICE double[5] = {lr, momentum | beta1, beta2 | alpha, eps, weight_decay}: Adam's bias corrections 1 - beta^t are formed
// in double as torch forms them on the host (an fp32 1 - 0.999^t is 3e-5 off at t = 1, which a bias tensor that starts at zero shows in full).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace idl_dev {

constexpr int KIND_SGD = 1, KIND_ADAM = 2, KIND_RMSPROP = 3;

// What one step's update needs, in the precision torch's kernels see it: the host-side Python floats rounded to fp32.
template <int KIND>
struct Coef {
    float lr, mu, wd;                             // SGD; RMSprop: these and eps, b2 = alpha, b2w = 1 - alpha
    float step, bc2s, eps, b1w, b2, b2w;          // Adam: lr / bc1, sqrt(bc2), eps, 1 - beta1, beta2, 1 - beta2
};

__device__ __forceinline__ double pow_int(double b, int64_t e)      // b^e, e >= 0 (wave-uniform: no divergence)
{
    double r = 1.0;
    while (e > 0) {
        if (e & 1) r *= b;
        b *= b;
        e >>= 1;
    }
    return r;
}

// hyper: the DEVICE double[5] above; step_in: the word that holds the number of steps taken so far (read for Adam only)
template <int KIND>
__device__ __forceinline__ Coef<KIND> make_coef(const double *hyper, const int64_t *step_in)
{
    Coef<KIND> c{};
    const double lr = hyper[0], h1 = hyper[1], h2 = hyper[2], eps = hyper[3], wd = hyper[4];
    c.wd = (float)wd;
    if constexpr (KIND == KIND_SGD) {
        c.lr = (float)lr; c.mu = (float)h1;
    } else if constexpr (KIND == KIND_RMSPROP) {
        c.lr = (float)lr; c.mu = (float)h1; c.eps = (float)eps; c.b2 = (float)h2; c.b2w = (float)(1.0 - h2);
    } else {
        const int64_t t = *step_in + 1;
        const double bc1 = 1.0 - pow_int(h1, t), bc2 = 1.0 - pow_int(h2, t);
        c.step = (float)(lr / bc1); c.bc2s = (float)sqrt(bc2); c.eps = (float)eps;
        c.b1w = (float)(1.0 - h1); c.b2 = (float)h2; c.b2w = (float)(1.0 - h2);
    }
    return c;
}

// torch.optim.SGD (momentum, weight decay; dampening 0, no nesterov): g' = g + wd p; buf = mu buf + g'; p -= lr buf -- a zero buf
// makes the first step buf = g', torch's clone.  torch.optim.Adam (no amsgrad): m.lerp_(g, 1 - b1); v = b2 v + (1 - b2) g g;
// p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps).  torch.optim.RMSprop (not centered) with a momentum buffer: v = alpha v + (1 - alpha) g' g';
// avg = sqrt(v) + eps; buf = mu buf + g' / avg; p -= lr buf (s1 = v, s2 = buf) -- mu = 0 makes buf = g' / avg, torch's addcdiv_ form.
template <int KIND>
__device__ __forceinline__ void opt_update(float g, float &p, float &s1, float &s2, const Coef<KIND> &c)
{
    g = fmaf(c.wd, p, g);
    if constexpr (KIND == KIND_SGD) {
        s1 = fmaf(c.mu, s1, g);
        p = fmaf(-c.lr, s1, p);
    } else if constexpr (KIND == KIND_RMSPROP) {
        s1 = fmaf(c.b2w * g, g, c.b2 * s1);
        const float avg = sqrtf(s1) + c.eps;
        s2 = fmaf(c.mu, s2, g / avg);
        p = fmaf(-c.lr, s2, p);
    } else {
        const float d = g - s1;
        s1 = c.b1w < 0.5f ? fmaf(c.b1w, d, s1) : g - d * (1.0f - c.b1w);      // (Tensor.lerp_'s two forms)
        s2 = fmaf(c.b2w * g, g, c.b2 * s2);
        const float denom = sqrtf(s2) / c.bc2s + c.eps;
        p = fmaf(-c.step, s1 / denom, p);
    }
}

}  // namespace idl_dev
