// Device helpers of the optimizer update kernels (optim.hip, optim_keras.hip): the launch shape, the device iteration
// count with its ticket rule, and the learning rate -- lr / (1 + decay*it) by value, or a schedule descriptor
// (lisec_lr_schedule) evaluated once per workgroup.
#pragma once
#include "common.h"

namespace lisec {
namespace {

constexpr int kOptBlocks = 1024;
constexpr int kOptThreads = 256;

// The iteration count of the step, read by every workgroup before any of them may advance it.
__device__ __forceinline__ long long read_iterations(const long long* state) {
    return __hip_atomic_load(&state[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// advance == 1: the workgroup that takes the last ticket increments state[0], i.e. after every workgroup has read it
// (state[1] is the ticket counter, 0 between launches).  advance == 0: the update of a PART of the variables ahead of
// the rest of the step; the count is left alone.
__device__ __forceinline__ void advance_iterations(long long* state, long long it) {
    __syncthreads();                                                   // every wave of this workgroup has read `it`
    if (threadIdx.x == 0) {
        const unsigned long long t = atomicAdd(reinterpret_cast<unsigned long long*>(&state[1]), 1ULL);
        if (t == (unsigned long long)gridDim.x - 1) {
            __hip_atomic_store(&state[1], 0LL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&state[0], it + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// lr_t = lr / (1 + decay*it), in double and rounded once: what the SGD-Nesterov kernel computes
__device__ __forceinline__ float decayed_lr(double lr, double decay, long long it) {
    return (float)(lr / (1.0 + decay * (double)it));
}

// schedule(it) of the descriptor (include/lisec_hip.h), in double: the arithmetic of tf.keras 2.4
// optimizers.schedules, with TF's order of operations.
__device__ double schedule_value(const lisec_lr_schedule* __restrict__ s, double step) {
    constexpr double kPi = 3.14159265358979323846;
    const double init = s->initial, ds = s->decay_steps;
    switch (s->kind) {
    case LISEC_LR_EXPONENTIAL: {
        double p = step / ds;
        if (s->flag) p = floor(p);
        return init * pow(s->decay_rate, p);
    }
    case LISEC_LR_PIECEWISE: {
        int nb = s->n_boundaries;
        nb = nb < 0 ? 0 : (nb > LISEC_LR_MAX_BOUNDARIES ? LISEC_LR_MAX_BOUNDARIES : nb);   // never read past the tables
        for (int i = 0; i < nb; ++i)
            if (step <= s->boundaries[i]) return s->values[i];
        return s->values[nb];
    }
    case LISEC_LR_POLYNOMIAL: {
        double d = ds, x = step;
        if (s->flag) d *= (x == 0.0 ? 1.0 : ceil(x / ds));
        else x = fmin(x, ds);
        return (init - s->end_learning_rate) * pow(1.0 - x / d, s->power) + s->end_learning_rate;
    }
    case LISEC_LR_INVERSE_TIME: {
        double p = step / ds;
        if (s->flag) p = floor(p);
        return init / (1.0 + s->decay_rate * p);
    }
    case LISEC_LR_COSINE: {
        const double f = fmin(step, ds) / ds;
        const double c = 0.5 * (1.0 + cos(kPi * f));
        return init * ((1.0 - s->alpha) * c + s->alpha);
    }
    case LISEC_LR_COSINE_RESTARTS: {
        double f = step / ds, i;
        const double tm = s->t_mul;
        if (tm == 1.0) {
            i = floor(f);
            f -= i;
        } else {
            i = floor(log(1.0 - f * (1.0 - tm)) / log(tm));
            const double ti = pow(tm, i);
            f = (f - (1.0 - ti) / (1.0 - tm)) / ti;
        }
        const double c = 0.5 * pow(s->m_mul, i) * (1.0 + cos(kPi * f));
        return init * ((1.0 - s->alpha) * c + s->alpha);
    }
    default:                                                           // LISEC_LR_CONSTANT
        return init;
    }
}

// lr_t = schedule(it) / (1 + decay*it), rounded once; a CONSTANT descriptor gives decayed_lr(lr, decay, it) bit for bit
__device__ __forceinline__ float scheduled_lr(const lisec_lr_schedule* __restrict__ s, long long it) {
    return decayed_lr(schedule_value(s, (double)it), s->decay, it);
}

// lr_t evaluated by one thread of the workgroup and shared through LDS: the double-precision schedule runs once per
// workgroup, ahead of the streaming loop.
__device__ __forceinline__ float workgroup_lr(const lisec_lr_schedule* __restrict__ s, long long it) {
    __shared__ float lr_shared;
    if (threadIdx.x == 0) lr_shared = scheduled_lr(s, it);
    __syncthreads();
    return lr_shared;
}

}  // namespace
}  // namespace lisec
