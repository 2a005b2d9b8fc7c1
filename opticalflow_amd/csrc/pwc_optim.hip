// Adam / AdamW parameter update with global-norm gradient clipping as three launches over all tensors of an optimizer
// (opticalflow_amd/optim.py; the reference's scripts end a step in clip_grad_norm_ + optimizer.step(), train2.py, or in
// GradScaler.step(optimizer), train.py):
//   1. optim_sqsum_kernel   one workgroup per chunk of kChunk gradient elements -> one fp64 partial of sum g^2 (products in fp64)
//   2. optim_finish_kernel  one workgroup: partials added in index order, total_norm, the clip coefficient, GradScaler's found_inf /
//                           grad_scale, the step record {step, beta1^step, beta2^step} advanced, the constants of the update written
//   3. optim_adam_kernel    same chunks: p, m, v updated in place from g, all in fp32
// Every tensor is cut into chunks of kChunk elements; the (tensor, chunk) list is built by the host once per parameter set.  The
// tensors' addresses come from two device tables: {p, m, v, numel} per tensor, which changes only with the parameter set, and
// the gradient pointers, which change whenever zero_grad(set_to_none=True) makes autograd allocate new ones.  A null gradient
// pointer leaves its tensor out of the step.  No atomics: a partial is a fixed-order sum of its chunk and the finish pass adds
// the partials one after the other, so the norm -- and with it every updated value -- is bit-reproducible.
//
// The fp32 arithmetic of the update is fixed (tests/optim_oracle.py restates it; -ffp-contract=off keeps it unfused), per element:
//   g = (g * inv_scale) * coef;   L2: g = g + wd * p;   decoupled: p = p * (1 - lr * wd)
//   m = m + (1 - b1) * (g - m);   v = v * b2 + (1 - b2) * (g * g)
//   p = p + (-step_size) * (m / (sqrt(v) / bc2_sqrt + eps))
// with step_size = lr / (1 - b1^step) and bc2_sqrt = sqrt(1 - b2^step) formed in fp64 and rounded once.  Division and square root
// are the correctly rounded ones: hipcc's default (-fhip-fp32-correctly-rounded-divide-sqrt) expands `/` and __builtin_sqrtf to
// IEEE results.  (__fsqrt_rn is NOT used: without OCML_BASIC_ROUNDED_OPERATIONS it is the 1-ulp native square root.)
#include <math.h>

#include "pwc_block_reduce.h"
#include "pwc_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 8192;                 // elements per workgroup: 8 float4 per lane and array
constexpr int kStage = 1024;                 // partials the finish pass stages in LDS at a time

struct TensorRec { float *p, *m, *v; int64_t numel; };                       // device table, one per tensor
struct ChunkRec { int tensor, chunk; };                                      // device table, one per workgroup
struct StepRec { double step, b1_pow, b2_pow; };                             // device-resident, one per parameter group
struct Consts { float step_size, bc2_sqrt, coef, inv_scale; int skip, pad[3]; };   // finish pass -> update pass, one per group
struct Hyper { float omb1, b2, omb2, eps, wd, decay; int mode; };            // mode 0: no weight decay, 1: L2, 2: decoupled
static_assert(sizeof(TensorRec) == 32 && sizeof(ChunkRec) == 8 && sizeof(StepRec) == 24 && sizeof(Consts) == 32, "optimizer table layouts");

__device__ __forceinline__ bool al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the tensors' addresses come out of a table in memory, so the compiler cannot know that they are global memory and would use flat
// accesses: say so
#define PWC_GLOBAL __attribute__((address_space(1)))
using gfloat = PWC_GLOBAL float;
typedef float v4f __attribute__((ext_vector_type(4)));     // float4 is a class, which cannot live in an address space
using gfloat4 = PWC_GLOBAL v4f;
__device__ __forceinline__ const gfloat *as_global(const float *p) { return (const gfloat *)p; }
__device__ __forceinline__ gfloat *as_global(float *p) { return (gfloat *)p; }

__global__ __launch_bounds__(kThreads) void optim_sqsum_kernel(const float *const *grads, const TensorRec *tensors,
                                                               const ChunkRec *chunks, double *partials) {
    __shared__ pwc::WaveLds<double, kThreads, 1> red;
    const int tid = threadIdx.x;
    const ChunkRec c = chunks[blockIdx.x];
    const float *gp = grads[c.tensor];
    double s[1] = {0.0};
    if (gp) {
        const int64_t off = (int64_t)c.chunk * kChunk, left = tensors[c.tensor].numel - off;
        const int n = left < kChunk ? (int)left : kChunk;
        const gfloat *g = as_global(gp + off);
        if (al16(gp)) {
            const gfloat4 *g4 = (const gfloat4 *)g;
            for (int i = tid; i < n / 4; i += kThreads) {
                const v4f x = g4[i];
                s[0] += (double)x.x * (double)x.x;
                s[0] += (double)x.y * (double)x.y;
                s[0] += (double)x.z * (double)x.z;
                s[0] += (double)x.w * (double)x.w;
            }
            for (int i = (n & ~3) + tid; i < n; i += kThreads) s[0] += (double)g[i] * (double)g[i];
        } else {
            for (int i = tid; i < n; i += kThreads) s[0] += (double)g[i] * (double)g[i];
        }
    }
    pwc::wave_block_sum(red, s);
    if (tid == 0) partials[blockIdx.x] = s[0];
}

__global__ __launch_bounds__(kThreads) void optim_finish_kernel(const double *partials, int64_t nchunks, int clip, float max_norm,
                                                                const float *found_inf, const float *grad_scale, double lr,
                                                                double beta1, double beta2, StepRec *rec, Consts *consts,
                                                                float *norm_out) {
    __shared__ double stage[kStage];
    const int tid = threadIdx.x;
    double sum = 0.0;
    if (clip) {
        for (int64_t base = 0; base < nchunks; base += kStage) {
            const int cnt = nchunks - base < kStage ? (int)(nchunks - base) : kStage;
            for (int i = tid; i < cnt; i += kThreads) stage[i] = partials[base + i];
            __syncthreads();
            if (tid == 0) {                                             // index order: one lane, one addition after the other;
#pragma unroll 8
                for (int i = 0; i < cnt; ++i) sum += stage[i];          // unrolled so that the LDS reads run ahead of the additions
            }
            __syncthreads();
        }
    }
    if (tid != 0) return;
    Consts k;
    k.inv_scale = grad_scale ? 1.0f / *grad_scale : 1.0f;
    k.coef = 1.0f;
    if (clip) {
        const float total = (float)sqrt(sum) * k.inv_scale;             // norm of the unscaled gradients
        const float c = max_norm / (total + 1e-6f);
        k.coef = c > 1.0f ? 1.0f : c;                                   // clamp(max=1): a NaN norm stays NaN, as in clip_grad_norm_
        *norm_out = total;
    }
    k.skip = (found_inf && *found_inf != 0.0f) ? 1 : 0;
    k.pad[0] = k.pad[1] = k.pad[2] = 0;
    StepRec r = *rec;
    if (!k.skip) {
        r.step += 1.0;
        r.b1_pow *= beta1;
        r.b2_pow *= beta2;
        *rec = r;
    }
    k.step_size = (float)(lr / (1.0 - r.b1_pow));
    k.bc2_sqrt = (float)sqrt(1.0 - r.b2_pow);
    *consts = k;
}

__device__ __forceinline__ void adam1(float &p, float g, float &m, float &v, const Consts &k, const Hyper &h) {
    g = g * k.inv_scale * k.coef;
    if (h.mode == 1) g = g + h.wd * p;
    else if (h.mode == 2) p = p * h.decay;
    m = m + h.omb1 * (g - m);
    v = v * h.b2 + h.omb2 * (g * g);
    p = p + (-k.step_size) * (m / (__builtin_sqrtf(v) / k.bc2_sqrt + h.eps));
}

__global__ __launch_bounds__(kThreads) void optim_adam_kernel(const float *const *grads, const TensorRec *tensors,
                                                              const ChunkRec *chunks, const Consts *consts, Hyper h) {
    const Consts k = *consts;
    if (k.skip) return;                                                  // GradScaler found an inf / NaN: nothing is written
    const int tid = threadIdx.x;
    const ChunkRec c = chunks[blockIdx.x];
    const float *gp = grads[c.tensor];
    if (!gp) return;
    const TensorRec t = tensors[c.tensor];
    const int64_t off = (int64_t)c.chunk * kChunk, left = t.numel - off;     // a chunk starts 32 KiB-aligned inside its tensor
    const int n = left < kChunk ? (int)left : kChunk;
    const gfloat *g = as_global(gp + off);
    gfloat *p = as_global(t.p + off), *m = as_global(t.m + off), *v = as_global(t.v + off);
    int done = 0;
    if (al16(gp) && al16(t.p) && al16(t.m) && al16(t.v)) {
        const gfloat4 *g4 = (const gfloat4 *)g;
        gfloat4 *p4 = (gfloat4 *)p, *m4 = (gfloat4 *)m, *v4 = (gfloat4 *)v;
#pragma unroll 2
        for (int i = tid; i < n / 4; i += kThreads) {
            const v4f gg = g4[i];
            v4f pp = p4[i], mm = m4[i], vv = v4[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float pe = pp[e], me = mm[e], ve = vv[e];
                adam1(pe, gg[e], me, ve, k, h);
                pp[e] = pe;
                mm[e] = me;
                vv[e] = ve;
            }
            p4[i] = pp;
            m4[i] = mm;
            v4[i] = vv;
        }
        done = n & ~3;
    }
    for (int i = done + tid; i < n; i += kThreads) {                     // the tail of an aligned chunk, or a whole unaligned one
        float pp = p[i], mm = m[i], vv = v[i];
        adam1(pp, g[i], mm, vv, k, h);
        p[i] = pp;
        m[i] = mm;
        v[i] = vv;
    }
}

// workspace: [nchunks fp64 partials][ngroups Consts]
inline Consts *consts_of(void *workspace, int64_t nchunks, int group) {
    return reinterpret_cast<Consts *>(static_cast<double *>(workspace) + nchunks) + group;
}

int check_tables(const char *who, const void *grads, const void *tensors, const void *chunks, int64_t chunk_begin, int64_t chunk_count,
                 int64_t nchunks) {
    if (!grads || !tensors || !chunks) PWC_FAIL(PWC_EINVAL, "%s: null table", who);
    if (pwc::misaligned({grads, tensors, chunks}, 8)) PWC_FAIL(PWC_EALIGN, "%s: tables need 8-byte alignment", who);
    if (chunk_begin < 0 || chunk_count <= 0 || chunk_begin + chunk_count > nchunks || chunk_count > 0x7fffffffLL)
        PWC_FAIL(PWC_EINVAL, "%s: chunks [%lld, +%lld) outside the table of %lld", who, (long long)chunk_begin, (long long)chunk_count,
                 (long long)nchunks);
    return PWC_OK;
}

int check_workspace(const char *who, const void *workspace, int64_t workspace_bytes, int64_t nchunks, int ngroups, int group) {
    if (nchunks <= 0 || ngroups <= 0 || group < 0 || group >= ngroups)
        PWC_FAIL(PWC_EINVAL, "%s: bad nchunks=%lld ngroups=%d group=%d", who, (long long)nchunks, ngroups, group);
    const int64_t need = pwc_optim_workspace_bytes(nchunks, ngroups);
    if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 7u))
        PWC_FAIL(PWC_EINVAL, "%s: workspace needs %lld bytes, 8-byte aligned", who, (long long)need);
    return PWC_OK;
}

}  // namespace

extern "C" int pwc_optim_chunk_elems(void) { return kChunk; }

extern "C" int64_t pwc_optim_workspace_bytes(int64_t nchunks, int ngroups) {
    if (nchunks <= 0 || ngroups <= 0 || nchunks > 0x7fffffffLL) return -1;
    return nchunks * (int64_t)sizeof(double) + (int64_t)ngroups * (int64_t)sizeof(Consts);
}

extern "C" int pwc_optim_grad_sqsum(const void *grads, const void *tensors, const void *chunks, int64_t nchunks, int ngroups,
                                    void *workspace, int64_t workspace_bytes, void *stream) {
    if (int rc = check_workspace("pwc_optim_grad_sqsum", workspace, workspace_bytes, nchunks, ngroups, 0)) return rc;
    if (int rc = check_tables("pwc_optim_grad_sqsum", grads, tensors, chunks, 0, nchunks, nchunks)) return rc;
    hipLaunchKernelGGL(optim_sqsum_kernel, dim3((unsigned)nchunks), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float *const *>(grads), static_cast<const TensorRec *>(tensors),
                       static_cast<const ChunkRec *>(chunks), static_cast<double *>(workspace));
    return pwc::check_launch("optim_sqsum_kernel");
}

extern "C" int pwc_optim_finish(void *workspace, int64_t workspace_bytes, int64_t nchunks, int ngroups, int group, int clip,
                                double max_norm, const void *found_inf, const void *grad_scale, double lr, double beta1,
                                double beta2, void *step_record, void *norm_out, void *stream) {
    if (int rc = check_workspace("pwc_optim_finish", workspace, workspace_bytes, nchunks, ngroups, group)) return rc;
    if (!step_record || (clip && !norm_out)) PWC_FAIL(PWC_EINVAL, "pwc_optim_finish: null pointer");
    if (pwc::misaligned({step_record}, 8) || pwc::misaligned({norm_out, found_inf, grad_scale}))
        PWC_FAIL(PWC_EALIGN, "pwc_optim_finish: step record needs 8-byte, the scalars 4-byte alignment");
    if (clip && !(max_norm > 0.0)) PWC_FAIL(PWC_EINVAL, "pwc_optim_finish: max_norm %g must be positive", max_norm);
    if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0))
        PWC_FAIL(PWC_EINVAL, "pwc_optim_finish: needs lr >= 0 and betas in [0, 1), got %g, %g, %g", lr, beta1, beta2);
    hipLaunchKernelGGL(optim_finish_kernel, dim3(1), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       static_cast<const double *>(workspace), nchunks, clip ? 1 : 0, (float)max_norm,
                       static_cast<const float *>(found_inf), static_cast<const float *>(grad_scale), lr, beta1, beta2,
                       static_cast<StepRec *>(step_record) + group, consts_of(workspace, nchunks, group), static_cast<float *>(norm_out));
    return pwc::check_launch("optim_finish_kernel");
}

extern "C" int pwc_optim_adam_update(const void *grads, const void *tensors, const void *chunks, int64_t nchunks, int64_t chunk_begin,
                                     int64_t chunk_count, int ngroups, int group, const void *workspace, int64_t workspace_bytes,
                                     double lr, double beta1, double beta2, double eps, double weight_decay, int decoupled,
                                     void *stream) {
    if (int rc = check_workspace("pwc_optim_adam_update", workspace, workspace_bytes, nchunks, ngroups, group)) return rc;
    if (int rc = check_tables("pwc_optim_adam_update", grads, tensors, chunks, chunk_begin, chunk_count, nchunks)) return rc;
    if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !(weight_decay >= 0.0))
        PWC_FAIL(PWC_EINVAL, "pwc_optim_adam_update: needs lr, eps, weight_decay >= 0 and betas in [0, 1)");
    Hyper h;
    h.omb1 = (float)(1.0 - beta1);
    h.b2 = (float)beta2;
    h.omb2 = (float)(1.0 - beta2);
    h.eps = (float)eps;
    h.wd = (float)weight_decay;
    h.decay = (float)(1.0 - lr * weight_decay);
    h.mode = weight_decay == 0.0 ? 0 : (decoupled ? 2 : 1);
    hipLaunchKernelGGL(optim_adam_kernel, dim3((unsigned)chunk_count), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float *const *>(grads), static_cast<const TensorRec *>(tensors),
                       static_cast<const ChunkRec *>(chunks) + chunk_begin,
                       consts_of(const_cast<void *>(workspace), nchunks, group), h);
    return pwc::check_launch("optim_adam_kernel");
}
