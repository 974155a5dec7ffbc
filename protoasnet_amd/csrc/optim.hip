// Training: the optimizer side of a step, one launch each.
//
//   pasn_adam_step       torch.optim.Adam's update of EVERY parameter that holds a gradient (the reference's `optimizer.step()`,
//                        Video_XProtoNet_e2e.py:137-142, over the parameter groups of XProtoNet_e2e.py:36-82)
//   pasn_grad_accumulate dst += src for a list of tensors (the undivided accumulation of the same loop, for the gradients that do not
//                        live in the training arena's flat buffer; the flat span itself goes through pasn_add_inplace)
//
// Both are driven by a job table in device memory, as pack.hip is: block b works on chunk block_chunk[b] of job block_job[b].  They are
// plain streaming code: Adam moves 28 bytes per element (p, g, m, v read; p, m, v written), the accumulation 12.  16-byte accesses when
// every pointer of the job is 16-byte aligned (a chunk starts at a multiple of OPTIM_CHUNK elements, so the job's alignment is the
// chunk's), 4-byte accesses otherwise: a view that starts at an odd storage offset is a legal input.
#include "common.h"

namespace pasn {

constexpr int OPTIM_CHUNK = 2048;  // elements per block (256 threads x 2 x 4)

// The job structs hand out generic pointers; everything they name is device memory, and saying so gives global_load / global_store
// instead of the flat forms.
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) f32x4 gf32x4;
typedef __attribute__((address_space(1))) unsigned long long gword;

struct AdamGroups {
    pasn_adam_group g[PASN_OPTIM_MAX_GROUPS];
};

// The scalars of one (job, step), as torch computes them: Python floats, i.e. double, rounded to fp32 where they meet a tensor.
struct AdamScalars {
    float w1, beta2, w2, neg_step_size, bc2_sqrt, eps, wd;
};

__device__ __forceinline__ double pow_int(double b, unsigned t) {  // b^t by squaring: <= 64 roundings in double, far below one fp32 ulp
    double r = 1.0;
    while (t) {
        if (t & 1u) r *= b;
        b *= b;
        t >>= 1;
    }
    return r;
}

__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, const AdamScalars& s) {
    if (s.wd != 0.0f) g = g + s.wd * p;                         // grad.add(param, alpha=weight_decay)
    m = m + s.w1 * (g - m);                                      // exp_avg.lerp_(grad, 1 - beta1), weight < 0.5
    v = v * s.beta2;                                             // exp_avg_sq.mul_(beta2)
    v = v + s.w2 * g * g;                                        //           .addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;           // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
    p = p + s.neg_step_size * (m / denom);                       // param.addcdiv_(exp_avg, denom, value=-step_size)
}

__device__ __forceinline__ bool aligned16(const void* a, const void* b, const void* c = nullptr, const void* d = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15u) == 0;
}

__global__ __launch_bounds__(256) void adam_step_kernel(const pasn_adam_job* __restrict__ jobs, const int* __restrict__ block_job,
                                                        const int* __restrict__ block_chunk, AdamGroups groups, unsigned stamp) {
    const pasn_adam_job j = jobs[block_job[blockIdx.x]];
    const int chunk = block_chunk[blockIdx.x];
    // The step word: t in the low half, the stamp of the call that last advanced it in the high half.  Every block of the job needs
    // t + 1, and one of them (chunk 0) stores it: a block that starts after that store sees this call's stamp and takes t as it is.
    // The word is read and written whole (one aligned 8-byte access), so no block can see half of an update.
    const unsigned long long word = __atomic_load_n((gword*)j.step, __ATOMIC_RELAXED);
    const unsigned t = (unsigned)(word >> 32) == stamp ? (unsigned)word : (unsigned)word + 1u;
    const pasn_adam_group h = groups.g[j.group];
    AdamScalars s;
    {
        const double bc1 = 1.0 - pow_int(h.beta1, t), bc2 = 1.0 - pow_int(h.beta2, t);
        s.w1 = (float)(1.0 - h.beta1);
        s.beta2 = (float)h.beta2;
        s.w2 = (float)(1.0 - h.beta2);
        s.neg_step_size = (float)(-(h.lr / bc1));
        s.bc2_sqrt = (float)sqrt(bc2);
        s.eps = (float)h.eps;
        s.wd = (float)h.weight_decay;
    }
    const long i0 = (long)chunk * OPTIM_CHUNK;
    const long end = i0 + OPTIM_CHUNK < j.n ? i0 + OPTIM_CHUNK : j.n;
    gfloat* __restrict__ P = (gfloat*)j.param;
    const gfloat* __restrict__ G = (const gfloat*)j.grad;
    gfloat* __restrict__ M = (gfloat*)j.exp_avg;
    gfloat* __restrict__ V = (gfloat*)j.exp_avg_sq;
    long scalar_from = i0;  // elements [scalar_from, end) go one by one
    if (aligned16(j.param, j.grad, j.exp_avg, j.exp_avg_sq)) {
        const long full = i0 + ((end - i0) & ~3L);  // whole groups of four inside the chunk
#pragma unroll
        for (int e = 0; e < OPTIM_CHUNK / 1024; ++e) {
            const long i = i0 + ((long)e * 256 + threadIdx.x) * 4;
            if (i + 4 > full) break;
            f32x4 p = *reinterpret_cast<const gf32x4*>(P + i);
            const f32x4 g = *reinterpret_cast<const gf32x4*>(G + i);
            f32x4 m = *reinterpret_cast<const gf32x4*>(M + i);
            f32x4 v = *reinterpret_cast<const gf32x4*>(V + i);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float pk = p[k], mk = m[k], vk = v[k];
                adam_element(pk, g[k], mk, vk, s);
                p[k] = pk, m[k] = mk, v[k] = vk;
            }
            *reinterpret_cast<gf32x4*>(P + i) = p;
            *reinterpret_cast<gf32x4*>(M + i) = m;
            *reinterpret_cast<gf32x4*>(V + i) = v;
        }
        scalar_from = full;
    }
    for (long i = scalar_from + threadIdx.x; i < end; i += 256) {
        float p = P[i], m = M[i], v = V[i];
        adam_element(p, G[i], m, v, s);
        P[i] = p, M[i] = m, V[i] = v;
    }
    if (chunk == 0 && threadIdx.x == 0) __atomic_store_n((gword*)j.step, ((unsigned long long)stamp << 32) | t, __ATOMIC_RELAXED);
}

__global__ __launch_bounds__(256) void grad_accumulate_kernel(const pasn_accum_job* __restrict__ jobs, const int* __restrict__ block_job,
                                                              const int* __restrict__ block_chunk) {
    const pasn_accum_job j = jobs[block_job[blockIdx.x]];
    const long i0 = (long)block_chunk[blockIdx.x] * OPTIM_CHUNK;
    const long end = i0 + OPTIM_CHUNK < j.n ? i0 + OPTIM_CHUNK : j.n;
    gfloat* __restrict__ D = (gfloat*)j.dst;
    const gfloat* __restrict__ S = (const gfloat*)j.src;
    long scalar_from = i0;
    if (aligned16(j.dst, j.src)) {
        const long full = i0 + ((end - i0) & ~3L);
#pragma unroll
        for (int e = 0; e < OPTIM_CHUNK / 1024; ++e) {
            const long i = i0 + ((long)e * 256 + threadIdx.x) * 4;
            if (i + 4 > full) break;
            *reinterpret_cast<gf32x4*>(D + i) = *reinterpret_cast<const gf32x4*>(D + i) + *reinterpret_cast<const gf32x4*>(S + i);
        }
        scalar_from = full;
    }
    for (long i = scalar_from + threadIdx.x; i < end; i += 256) D[i] = D[i] + S[i];
}

// The tables live in device memory; `host` is the caller's host copy of the job table, checked here before anything is launched: the
// block count must be the one the jobs' sizes give, so that no block can index past a job.
static int arg_error(const char* entry, const std::string& msg) {
    set_error(std::string(entry) + ": " + msg);
    return PASN_ERR_ARG;
}

template <typename Job, typename Check>
static int check_tables(const char* entry, const Job* jobs, const Job* host, int njobs, const int* block_job, const int* block_chunk, int nblocks,
                        Check per_job) {
    if (!(jobs && host && block_job && block_chunk)) return arg_error(entry, "null table");
    if (njobs <= 0 || nblocks <= 0) return arg_error(entry, "empty job table");
    long blocks = 0;
    for (int i = 0; i < njobs; ++i) {
        if (host[i].n <= 0) return arg_error(entry, "job " + std::to_string(i) + ": n must be positive");
        const std::string bad = per_job(host[i]);
        if (!bad.empty()) return arg_error(entry, "job " + std::to_string(i) + ": " + bad);
        blocks += (host[i].n + OPTIM_CHUNK - 1) / OPTIM_CHUNK;
    }
    if (blocks != nblocks)
        return arg_error(entry, "nblocks = " + std::to_string(nblocks) + " but the jobs' sizes give " + std::to_string(blocks) + " chunks");
    return PASN_OK;
}

}  // namespace pasn

extern "C" int pasn_optim_chunk(void) { return pasn::OPTIM_CHUNK; }

extern "C" int pasn_adam_step(const pasn_adam_job* jobs, const pasn_adam_job* jobs_host, int njobs, const int* block_job, const int* block_chunk,
                              int nblocks, const pasn_adam_group* groups, int ngroups, unsigned stamp, void* stream) {
    using namespace pasn;
    PASN_REQUIRE(groups, "null groups");
    PASN_REQUIRE(ngroups >= 1 && ngroups <= PASN_OPTIM_MAX_GROUPS,
                 std::to_string(ngroups) + " parameter groups; the argument block holds " + std::to_string(PASN_OPTIM_MAX_GROUPS));
    PASN_REQUIRE(stamp != 0, "stamp 0 is the value of a step word no call has advanced");
    const int rc = check_tables("pasn_adam_step", jobs, jobs_host, njobs, block_job, block_chunk, nblocks, [&](const pasn_adam_job& j) {
        if (!(j.param && j.grad && j.exp_avg && j.exp_avg_sq && j.step)) return std::string("null pointer");
        if (j.group < 0 || j.group >= ngroups) return "group " + std::to_string(j.group) + " of " + std::to_string(ngroups);
        return std::string();
    });
    if (rc != PASN_OK) return rc;
    AdamGroups gs = {};
    for (int i = 0; i < ngroups; ++i) gs.g[i] = groups[i];
    hipLaunchKernelGGL(adam_step_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, jobs, block_job, block_chunk, gs, stamp);
    return check_launch("adam_step_kernel");
}

extern "C" int pasn_grad_accumulate(const pasn_accum_job* jobs, const pasn_accum_job* jobs_host, int njobs, const int* block_job,
                                    const int* block_chunk, int nblocks, void* stream) {
    using namespace pasn;
    const int rc = check_tables("pasn_grad_accumulate", jobs, jobs_host, njobs, block_job, block_chunk, nblocks,
                                [](const pasn_accum_job& j) { return j.dst && j.src ? std::string() : std::string("null pointer"); });
    if (rc != PASN_OK) return rc;
    hipLaunchKernelGGL(grad_accumulate_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, jobs, block_job, block_chunk);
    return check_launch("grad_accumulate_kernel");
}
