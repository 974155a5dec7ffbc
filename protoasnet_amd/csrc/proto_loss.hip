// proto_loss.hip -- the reference's training loss recipe (src/loss/loss.py:23-254, 323-371 as applied by XProtoNet_Base.py:54-81 and
// Video_XProtoNet_e2e.py:86-110) and the per-batch epoch statistics (Video_XProtoNet_e2e.py:112-153) in two launches forward and two
// launches backward.
//
// Forward.  Launch 1 (only when the map norm or the orthogonality term is on) has two kinds of blocks: map blocks, one WAVE per
// (clip, prototype) row of the occurrence maps, read the row with 16-byte loads and leave its p-norm in the workspace; prototype blocks,
// one per prototype i, leave sum_{j > i, same group} cos(p_i, p_j).  Launch 2 is ONE block: the cross entropy (plain or with the learned
// abstention output), the cluster / separation costs, the masked norm of the last layer, the sums of the two partial arrays, the seven
// weighted terms, their total, and -- when asked for -- the confusion-matrix counts and the running term sums of the epoch.
//
// Backward.  Launch 1: block 0 writes d_logits, d_similarities and d_fc_weight; block 1 + i writes the orthogonality gradient of
// prototype i.  Launch 2: one wave per map row writes d_occurrence_map in the map's dtype.  The upstream gradient is read from the device.
//
// Every sum is taken in a fixed order (lane-strided partials, xor shuffles, waves combined in index order), in fp64: the tensors are tiny
// next to a trunk launch and the result then sits within the reference's own fp32 rounding.  No floating-point atomics; the confusion
// matrix uses integer atomics, which do not depend on the order of arrival.  Two runs on the same inputs are bitwise equal.
// Subgradients as autograd takes them: sign(0) = 0, an all-zero row under p = 2 gets a zero gradient, a tied per-class maximum
// (minimum) sends its gradient to the first index.
#include "common.h"

namespace pasn {

constexpr int PL_THREADS = 256;
constexpr int PL_WAVES = PL_THREADS / 64;
constexpr int PL_MAX_GROUP = 2048;  // prototypes of one orthogonality group: two fp64 coefficient rows of LDS in the backward

__device__ __forceinline__ double pl_wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// sum over the block, the same value in every thread; `red` holds PL_WAVES doubles
__device__ __forceinline__ double pl_block_sum(double v, double* red) {
    v = pl_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ int pl_clamp_target(long t, int k) { return t < 0 ? 0 : (t >= k ? k - 1 : (int)t); }

// ---- one map row: sum |x| (p = 1) or sum x^2 (p = 2) over S elements, by one wave, 16 bytes per lane and load where the row allows ----
template <typename T>
__device__ __forceinline__ double pl_row_moment(const T* __restrict__ row, long S, int p, bool vec, int lane) {
    constexpr int V = 16 / sizeof(T);
    double acc = 0.0;
    long done = 0;
    if (vec) {
        const long nv = S / V;
        for (long v = lane; v < nv; v += 64) {
            float x[V];
            if constexpr (V == 8) load8(row + v * V, x);
            else load4(row + v * V, x);
#pragma unroll
            for (int j = 0; j < V; ++j) acc += p == 1 ? (double)fabsf(x[j]) : (double)x[j] * (double)x[j];
        }
        done = nv * V;
    }
    for (long e = done + lane; e < S; e += 64) {
        const float x = (float)row[e];
        acc += p == 1 ? (double)fabsf(x) : (double)x * (double)x;
    }
    return pl_wave_sum(acc);
}

// cos(a, b) pieces of one prototype pair by one wave: dot(a, b) and |b|^2
__device__ __forceinline__ void pl_pair(const float* __restrict__ a, const float* __restrict__ b, int D, int lane, double& dot, double& bb) {
    double d = 0.0, n = 0.0;
    for (int k = lane; k < D; k += 64) {
        const double x = a[k], y = b[k];
        d += x * y;
        n += y * y;
    }
    dot = pl_wave_sum(d);
    bb = pl_wave_sum(n);
}

// torch.nn.functional.cosine_similarity divides each vector by max(|v|, eps), eps = 1e-8
__device__ __forceinline__ double pl_clamped(double norm) { return norm > 1e-8 ? norm : 1e-8; }

template <typename T>
__global__ __launch_bounds__(PL_THREADS) void proto_loss_partials_kernel(const T* __restrict__ occ, const float* __restrict__ protos,
                                                                         pasn_proto_loss_desc d, int map_blocks, bool vec,
                                                                         float* __restrict__ rownorm, float* __restrict__ ortho_part) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if ((int)blockIdx.x < map_blocks) {
        const long row = (long)blockIdx.x * PL_WAVES + wave;
        if (row >= (long)d.N * d.P) return;
        const double m = pl_row_moment(occ + row * d.S, d.S, d.map_p, vec, lane);
        if (lane == 0) rownorm[row] = (float)(d.map_p == 1 ? m : sqrt(m));
        return;
    }
    __shared__ double red[PL_WAVES];
    const int i = (int)blockIdx.x - map_blocks;
    const int G = d.ortho_mode == 0 ? d.P / d.C : d.P;
    const int hi = (i / G + 1) * G;  // one past the last prototype of i's group
    const float* a = protos + (long)i * d.D;
    double aa, unused;
    pl_pair(a, a, d.D, lane, unused, aa);
    const double na = pl_clamped(sqrt(aa));
    double part = 0.0;
    for (int j = i + 1 + wave; j < hi; j += PL_WAVES) {
        double dot, bb;
        pl_pair(a, protos + (long)j * d.D, d.D, lane, dot, bb);
        part += dot / (na * pl_clamped(sqrt(bb)));
    }
    if (lane == 0) red[wave] = part;
    __syncthreads();
    if (tid == 0) ortho_part[i] = (float)((red[0] + red[1]) + (red[2] + red[3]));
}

// per-class extreme of one row of scores: value and FIRST index of the class's group
__device__ __forceinline__ void pl_group_extreme(const float* __restrict__ row, int G, bool smallest, float& best, int& arg) {
    best = row[0];
    arg = 0;
    for (int q = 1; q < G; ++q) {
        const float v = row[q];
        if (best != best) break;  // a NaN wins and stays, as in torch.max / torch.min
        if (v != v || (smallest ? v < best : v > best)) {
            best = v;
            arg = q;
        }
    }
}

// the cross entropy of one row in fp64: loss parts and, when dl != NULL, d(row loss) / d logits scaled by `scale`
__device__ __forceinline__ void pl_ce_row(const float* __restrict__ lg, int K, int t, int mode, double ab_weight, double& pred, double& abst,
                                          float* __restrict__ dl, double scale) {
    const int Kc = mode == 0 ? K : K - 1;  // classes of the class softmax
    double m = lg[0];
    for (int k = 1; k < Kc; ++k) m = fmax(m, (double)lg[k]);
    double s = 0.0;
    for (int k = 0; k < Kc; ++k) s += exp((double)lg[k] - m);
    const double ct = exp((double)lg[t] - m) / s;
    abst = 0.0;
    if (mode == 0) {
        pred = -((double)lg[t] - m - log(s));
        if (dl)
            for (int k = 0; k < K; ++k) dl[k] = (float)(scale * (exp((double)lg[k] - m) / s - (k == t ? 1.0 : 0.0)));
        return;
    }
    const double la = lg[Kc];
    double a;
    if (mode == 1) {  // joined: the abstention output takes part in one softmax over all K columns
        const double m2 = fmax(m, la);
        const double s2 = s * exp(m - m2) + exp(la - m2);
        a = exp(la - m2) / s2;
    } else {  // separate: its own sigmoid
        a = 1.0 / (1.0 + exp(-la));
    }
    const double vt = (1.0 - a) * ct + a;  // virtual prediction of the target class (loss.py:361)
    pred = -log(vt);
    abst = -log(1.0 - a);
    if (!dl) return;
    const double dv = -1.0 / vt;                                    // d pred / d vt
    const double da = dv * (1.0 - ct) + ab_weight / (1.0 - a);      // d row / d a
    for (int k = 0; k < Kc; ++k) {
        const double ck = exp((double)lg[k] - m) / s;
        double g = dv * (1.0 - a) * ct * ((k == t ? 1.0 : 0.0) - ck);
        if (mode == 1) {
            const double m2 = fmax(m, la);
            const double s2 = s * exp(m - m2) + exp(la - m2);
            g += da * a * (-(exp((double)lg[k] - m2) / s2));
        }
        dl[k] = (float)(scale * g);
    }
    dl[Kc] = (float)(scale * da * a * (1.0 - a));  // both paths: d a / d la = a (1 - a)
}

// coefficient of the per-class extreme of class c for a row whose (clamped) label is t: cluster on the own class, separation on the others
__device__ __forceinline__ double pl_score_coef(const pasn_proto_loss_desc& d, int c, int t, double rc, double rs) {
    const double sgn = d.patch ? -1.0 : 1.0;  // ProtoPNet costs act on distances: minimum, opposite signs (loss.py:37-95)
    if (c == t) return -sgn * (double)d.w_cluster * rc;
    if (d.sep_abstain && c == d.C - 1) return 0.0;  // the abstention prototypes are never penalised (loss.py:169-171)
    return sgn * (double)d.w_sep * rs;
}

__global__ __launch_bounds__(PL_THREADS) void proto_loss_finish_kernel(const float* __restrict__ logits, const float* __restrict__ sim,
                                                                       const int64_t* __restrict__ target, const float* __restrict__ fc_w,
                                                                       const float* __restrict__ fc_mask, const float* __restrict__ transform,
                                                                       pasn_proto_loss_desc d, const float* __restrict__ rownorm,
                                                                       const float* __restrict__ ortho_part, float* __restrict__ terms,
                                                                       float* __restrict__ loss, unsigned long long* __restrict__ cm,
                                                                       float* __restrict__ loss_sum) {
    __shared__ double red[PL_WAVES];
    const int tid = threadIdx.x;
    double ce = 0.0, ortho = 0.0, mapn = 0.0, fc = 0.0;
    if (d.w_ce != 0.0f) {
        const int Kc = d.ce_mode == 0 ? d.K : d.K - 1;
        double part = 0.0;
        for (int n = tid; n < d.N; n += PL_THREADS) {
            double pred, abst;
            pl_ce_row(logits + (long)n * d.K, d.K, pl_clamp_target(target[n], Kc), d.ce_mode, d.ab_weight, pred, abst, nullptr, 0.0);
            part += pred + (double)d.ab_weight * abst;
        }
        ce = pl_block_sum(part, red) * (d.ce_reduction == 0 ? 1.0 / d.N : 1.0) * (double)d.w_ce;
    }
    double cluster = 0.0, sep = 0.0;
    if (d.w_cluster != 0.0f || d.w_sep != 0.0f) {
        const int G = d.P / d.C;
        double pc = 0.0, ps = 0.0;
        for (int n = tid; n < d.N; n += PL_THREADS) {
            const int t = pl_clamp_target(target[n], d.C);
            for (int c = 0; c < d.C; ++c) {
                float best;
                int arg;
                pl_group_extreme(sim + (long)n * d.P + (long)c * G, G, d.patch != 0, best, arg);
                const double k = pl_score_coef(d, c, t, 1.0, 1.0);
                if (c == t) pc += k * (double)best;
                else ps += k * (double)best;
            }
        }
        cluster = d.w_cluster != 0.0f ? pl_block_sum(pc, red) * (d.cluster_reduction == 0 ? 1.0 / d.N : 1.0) : 0.0;
        sep = d.w_sep != 0.0f ? pl_block_sum(ps, red) * (d.sep_reduction == 0 ? 1.0 / d.N : 1.0) : 0.0;
    }
    if (d.w_ortho != 0.0f) {
        double part = 0.0;
        for (int i = tid; i < d.P; i += PL_THREADS) part += (double)ortho_part[i];
        ortho = pl_block_sum(part, red) * (double)d.w_ortho;
    }
    if (d.w_map != 0.0f) {
        double part = 0.0;
        const long rows = (long)d.N * d.P;
        for (long r = tid; r < rows; r += PL_THREADS) part += (double)rownorm[r];
        mapn = pl_block_sum(part, red) * (d.map_reduction == 0 ? 1.0 / d.N : 1.0) * (double)d.w_map;
    }
    if (d.w_fc != 0.0f) {
        double part = 0.0;
        const long n = (long)d.fc_rows * d.P;
        for (long e = tid; e < n; e += PL_THREADS) {
            const double x = (double)(fc_mask ? fc_mask[e] * fc_w[e] : fc_w[e]);
            part += d.fc_p == 1 ? fabs(x) : x * x;
        }
        const double m = pl_block_sum(part, red);
        fc = (d.fc_p == 1 ? m : sqrt(m)) * (double)d.w_fc;
    }
    if (cm) {  // rows: the clamped label, columns: the first largest real-class logit (torch.argmax on the eager path)
        for (int n = tid; n < d.N; n += PL_THREADS) {
            const float* lg = logits + (long)n * d.K;
            float best = lg[0];
            int arg = 0;
            for (int k = 1; k < d.K_real && best == best; ++k) {
                const float v = lg[k];
                if (v != v || v > best) {
                    best = v;
                    arg = k;
                }
            }
            atomicAdd(&cm[(long)pl_clamp_target(target[n], d.K_real) * d.K_real + arg], 1ull);
        }
    }
    if (tid != 0) return;
    const float t[7] = {(float)ce, (float)cluster, (float)sep, (float)ortho, (float)mapn, transform ? transform[0] : 0.0f, (float)fc};
    float total = 0.0f;
    for (int j = 0; j < 7; ++j) {  // the order sum(terms) adds in
        terms[j] = t[j];
        total += t[j];
        if (loss_sum) loss_sum[j] += t[j];
    }
    loss[0] = total;
}

__global__ __launch_bounds__(PL_THREADS) void proto_loss_bwd_small_kernel(const float* __restrict__ grad_out, const float* __restrict__ logits,
                                                                          const float* __restrict__ sim, const int64_t* __restrict__ target,
                                                                          const float* __restrict__ protos, const float* __restrict__ fc_w,
                                                                          const float* __restrict__ fc_mask, pasn_proto_loss_desc d,
                                                                          float* __restrict__ d_logits, float* __restrict__ d_sim,
                                                                          float* __restrict__ d_protos, float* __restrict__ d_fc_w) {
    extern __shared__ double pl_coef[];  // prototype blocks: [G] 1 / (|p_i| |p_j|), [G] dot(p_i, p_j) / (|p_i|^2 |p_j|)
    __shared__ double red[PL_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double g = (double)grad_out[0];
    if (blockIdx.x > 0) {
        const int i = (int)blockIdx.x - 1;
        float* out = d_protos + (long)i * d.D;
        if (d.w_ortho == 0.0f) {
            for (int k = tid; k < d.D; k += PL_THREADS) out[k] = 0.0f;
            return;
        }
        const int G = d.ortho_mode == 0 ? d.P / d.C : d.P;
        const int lo = (i / G) * G;
        const float* a = protos + (long)i * d.D;
        double aa, unused;
        pl_pair(a, a, d.D, lane, unused, aa);
        const double na = sqrt(aa), nca = pl_clamped(na);
        double* ca = pl_coef;
        double* cb = pl_coef + G;
        for (int q = wave; q < G; q += PL_WAVES) {
            double dot, bb;
            pl_pair(a, protos + (long)(lo + q) * d.D, d.D, lane, dot, bb);
            const double ncb = pl_clamped(sqrt(bb));
            if (lane == 0) {
                ca[q] = lo + q == i ? 0.0 : 1.0 / (nca * ncb);
                cb[q] = lo + q == i ? 0.0 : dot / (nca * nca * ncb);
            }
        }
        __syncthreads();
        double sb = 0.0;
        for (int q = 0; q < G; ++q) sb += cb[q];
        const double self = na > 0.0 ? sb / na : 0.0;  // the norm's own gradient a / |a|, zero at the origin
        const double w = g * (double)d.w_ortho;
        for (int k = tid; k < d.D; k += PL_THREADS) {
            double acc = 0.0;
            for (int q = 0; q < G; ++q) acc += ca[q] * (double)protos[(long)(lo + q) * d.D + k];
            out[k] = (float)(w * (acc - self * (double)a[k]));
        }
        return;
    }
    if (d_logits) {
        const int Kc = d.ce_mode == 0 ? d.K : d.K - 1;
        const double scale = g * (double)d.w_ce * (d.ce_reduction == 0 ? 1.0 / d.N : 1.0);
        for (int n = tid; n < d.N; n += PL_THREADS) {
            float* dl = d_logits + (long)n * d.K;
            if (d.w_ce == 0.0f) {
                for (int k = 0; k < d.K; ++k) dl[k] = 0.0f;
                continue;
            }
            double pred, abst;
            pl_ce_row(logits + (long)n * d.K, d.K, pl_clamp_target(target[n], Kc), d.ce_mode, d.ab_weight, pred, abst, dl, scale);
        }
    }
    if (d_sim) {
        const int G = d.P / d.C;
        const double rc = d.w_cluster != 0.0f ? (d.cluster_reduction == 0 ? 1.0 / d.N : 1.0) : 0.0;
        const double rs = d.w_sep != 0.0f ? (d.sep_reduction == 0 ? 1.0 / d.N : 1.0) : 0.0;
        for (int e = tid; e < d.N * d.C; e += PL_THREADS) {
            const int n = e / d.C, c = e - n * d.C;
            const long base = (long)n * d.P + (long)c * G;
            float best;
            int arg = -1;
            if (rc != 0.0 || rs != 0.0) pl_group_extreme(sim + base, G, d.patch != 0, best, arg);
            const float k = (float)(g * pl_score_coef(d, c, pl_clamp_target(target[n], d.C), rc, rs));
            for (int q = 0; q < G; ++q) d_sim[base + q] = q == arg ? k : 0.0f;
        }
    }
    if (d_fc_w) {
        const long n = (long)d.fc_rows * d.P;
        double norm = 0.0;
        if (d.w_fc != 0.0f && d.fc_p == 2) {
            double part = 0.0;
            for (long e = tid; e < n; e += PL_THREADS) {
                const double x = (double)(fc_mask ? fc_mask[e] * fc_w[e] : fc_w[e]);
                part += x * x;
            }
            norm = sqrt(pl_block_sum(part, red));
        }
        const double w = g * (double)d.w_fc;
        for (long e = tid; e < n; e += PL_THREADS) {
            const double mk = fc_mask ? (double)fc_mask[e] : 1.0;
            const double x = mk * (double)fc_w[e];
            double v = 0.0;
            if (d.w_fc != 0.0f) v = d.fc_p == 1 ? (x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0)) : (norm > 0.0 ? x / norm : 0.0);
            d_fc_w[e] = (float)(w * v * mk);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(PL_THREADS) void proto_loss_bwd_map_kernel(const float* __restrict__ grad_out, const T* __restrict__ occ,
                                                                        const float* __restrict__ rownorm, pasn_proto_loss_desc d, bool vec,
                                                                        T* __restrict__ d_occ) {
    constexpr int V = 16 / sizeof(T);
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * PL_WAVES + (threadIdx.x >> 6);
    if (row >= (long)d.N * d.P) return;
    const T* src = occ + row * d.S;
    T* dst = d_occ + row * d.S;
    if (d.w_map == 0.0f) {  // the term is off: zeros, nothing is read
        for (long e = lane; e < d.S; e += 64) dst[e] = (T)0.0f;
        return;
    }
    float k;  // p = 1: the coefficient of sign(x); p = 2: of x
    const double c = (double)grad_out[0] * (double)d.w_map * (d.map_reduction == 0 ? 1.0 / d.N : 1.0);
    if (d.map_p == 1) k = (float)c;
    else k = rownorm[row] > 0.0f ? (float)(c / (double)rownorm[row]) : 0.0f;
    const bool l1 = d.map_p == 1;
    long done = 0;
    if (vec) {
        const long nv = d.S / V;
        for (long v = lane; v < nv; v += 64) {
            float x[V];
            if constexpr (V == 8) load8(src + v * V, x);
            else load4(src + v * V, x);
#pragma unroll
            for (int j = 0; j < V; ++j) x[j] = l1 ? (x[j] > 0.0f ? k : (x[j] < 0.0f ? -k : 0.0f)) : k * x[j];
            if constexpr (V == 8) store8(dst + v * V, x);
            else store4(dst + v * V, x);
        }
        done = nv * V;
    }
    for (long e = done + lane; e < d.S; e += 64) {
        const float x = (float)src[e];
        dst[e] = (T)(l1 ? (x > 0.0f ? k : (x < 0.0f ? -k : 0.0f)) : k * x);
    }
}

static bool pl_vec_ok(const void* a, const void* b, long S, size_t esize) {
    return (S * (long)esize) % 16 == 0 && ((uintptr_t)a & 15) == 0 && ((uintptr_t)b & 15) == 0;
}

// the checks both entry points share; `need_*`: the operand is read by this call
static int pl_check(const pasn_proto_loss_desc* d, const char* who) {
    auto bad = [&](const char* msg) {
        set_error(std::string(who) + ": " + msg);
        return PASN_ERR_ARG;
    };
    if (!d) return bad("the descriptor is required");
    if (d->N < 1 || d->K < 1 || d->P < 1) return bad("N, K and P must be positive");
    if (d->ce_mode < 0 || d->ce_mode > 2) return bad("unknown cross-entropy mode (0 plain, 1 abstain joined, 2 abstain separate)");
    if (d->w_ce != 0.0f && d->ce_mode != 0 && d->K - 1 < 2) return bad("CeLossAbstain input must have >= 2 classes not including abstention");
    if (d->w_ce != 0.0f && d->ce_mode == 0 && d->K < 2) return bad("the cross entropy needs at least 2 classes");
    for (int r : {d->ce_reduction, d->cluster_reduction, d->sep_reduction, d->map_reduction})
        if (r != 0 && r != 1) return bad("unknown reduction (0 mean, 1 sum)");
    if (d->w_map != 0.0f && d->map_p != 1 && d->map_p != 2) return bad("the map norm is computed for p = 1 and p = 2");
    if (d->w_fc != 0.0f && d->fc_p != 1 && d->fc_p != 2) return bad("the last-layer norm is computed for p = 1 and p = 2");
    if (d->ortho_mode != 0 && d->ortho_mode != 1) return bad("unknown orthogonality mode (0 per_class, 1 all)");
    const bool grouped = d->w_cluster != 0.0f || d->w_sep != 0.0f || (d->w_ortho != 0.0f && d->ortho_mode == 0);
    if (grouped && (d->C < 1 || d->P % d->C != 0)) return bad("P must be divisible by the number of prototype classes");
    if (d->w_ortho != 0.0f && d->D < 1) return bad("D must be positive");
    if (d->w_map != 0.0f && d->S < 1) return bad("S must be positive");
    if (d->w_map != 0.0f && d->map_dtype != PASN_F32 && d->map_dtype != PASN_BF16) return bad("the maps are fp32 or bf16");
    if (d->w_fc != 0.0f && d->fc_rows < 1) return bad("fc_rows must be positive");
    if ((long)d->N * d->P > (1L << 30)) return bad("N * P is too large");
    return PASN_OK;
}

}  // namespace pasn

using namespace pasn;

extern "C" int pasn_proto_loss_fwd(const float* logits, const float* scores, const int64_t* target, const float* protos, const void* occ,
                                   const float* fc_w, const float* fc_mask, const float* transform_term, float* terms, float* loss,
                                   float* workspace, int64_t* cm, float* loss_sum, const pasn_proto_loss_desc* d, void* stream) {
    if (const int rc = pl_check(d, __func__)) return rc;
    PASN_REQUIRE(terms && loss, "terms and loss are required");
    PASN_REQUIRE(d->w_ce == 0.0f || (logits && target), "the cross entropy needs logits and target");
    PASN_REQUIRE((d->w_cluster == 0.0f && d->w_sep == 0.0f) || (scores && target), "the cluster / separation costs need the scores and target");
    PASN_REQUIRE(d->w_ortho == 0.0f || (protos && workspace), "the orthogonality term needs the prototypes and the workspace");
    PASN_REQUIRE(d->w_map == 0.0f || (occ && workspace), "the map norm needs the maps and the workspace");
    PASN_REQUIRE(d->w_fc == 0.0f || fc_w, "the last-layer norm needs the weight");
    PASN_REQUIRE(!cm || (logits && target && d->K_real >= 1 && d->K_real <= d->K), "the confusion matrix needs logits, target and K_real in [1, K]");
    hipStream_t s = (hipStream_t)stream;
    float* rownorm = workspace;
    float* ortho_part = workspace ? workspace + (size_t)d->N * d->P : nullptr;
    const int map_blocks = d->w_map != 0.0f ? ceil_div((long)d->N * d->P, PL_WAVES) : 0;
    const int proto_blocks = d->w_ortho != 0.0f ? d->P : 0;
    if (map_blocks + proto_blocks > 0) {
        if (d->w_map != 0.0f && d->map_dtype == PASN_BF16)
            hipLaunchKernelGGL(proto_loss_partials_kernel<__bf16>, dim3(map_blocks + proto_blocks), dim3(PL_THREADS), 0, s,
                               static_cast<const __bf16*>(occ), protos, *d, map_blocks, pl_vec_ok(occ, occ, d->S, 2), rownorm, ortho_part);
        else
            hipLaunchKernelGGL(proto_loss_partials_kernel<float>, dim3(map_blocks + proto_blocks), dim3(PL_THREADS), 0, s,
                               static_cast<const float*>(occ), protos, *d, map_blocks, map_blocks > 0 && pl_vec_ok(occ, occ, d->S, 4), rownorm,
                               ortho_part);
    }
    hipLaunchKernelGGL(proto_loss_finish_kernel, dim3(1), dim3(PL_THREADS), 0, s, logits, scores, target, fc_w, fc_mask, transform_term, *d,
                       rownorm, ortho_part, terms, loss, reinterpret_cast<unsigned long long*>(cm), loss_sum);
    return check_launch("proto_loss_fwd");
}

extern "C" int pasn_proto_loss_bwd(const float* grad_loss, const float* logits, const float* scores, const int64_t* target, const float* protos,
                                   const void* occ, const float* fc_w, const float* fc_mask, const float* workspace, float* d_logits,
                                   float* d_scores, float* d_protos, void* d_occ, float* d_fc_w, const pasn_proto_loss_desc* d, void* stream) {
    if (const int rc = pl_check(d, __func__)) return rc;
    PASN_REQUIRE(grad_loss, "the upstream gradient (a device scalar) is required");
    PASN_REQUIRE(!d_logits || d->w_ce == 0.0f || (logits && target), "d_logits needs logits and target");
    PASN_REQUIRE(!d_scores || (d->w_cluster == 0.0f && d->w_sep == 0.0f) || (scores && target), "d_scores needs the scores and target");
    PASN_REQUIRE(!d_scores || (d->C >= 1 && d->P % d->C == 0), "P must be divisible by the number of prototype classes");
    PASN_REQUIRE(!d_protos || d->w_ortho == 0.0f || protos, "d_prototype_vectors needs the prototypes");
    PASN_REQUIRE(!d_protos || d->D >= 1, "D must be positive");
    PASN_REQUIRE(!d_occ || d->w_map == 0.0f || (occ && workspace), "d_occurrence_map needs the maps and the forward's workspace");
    PASN_REQUIRE(!d_occ || (d->S >= 1 && (d->map_dtype == PASN_F32 || d->map_dtype == PASN_BF16)), "the maps are fp32 or bf16 rows of S >= 1 elements");
    PASN_REQUIRE(!d_fc_w || (d->fc_rows >= 1 && (d->w_fc == 0.0f || fc_w)), "d_fc_weight needs the weight and fc_rows");
    hipStream_t s = (hipStream_t)stream;
    if (d_logits || d_scores || d_protos || d_fc_w) {
        const int G = d->ortho_mode == 0 && d->C >= 1 && d->P % d->C == 0 ? d->P / d->C : d->P;
        if (d_protos && d->w_ortho != 0.0f && G > PL_MAX_GROUP) {
            set_error("pasn_proto_loss_bwd: more than 2048 prototypes in one orthogonality group is not supported (LDS)");
            return PASN_ERR_UNSUPPORTED;
        }
        const size_t lds = d_protos && d->w_ortho != 0.0f ? (size_t)2 * G * sizeof(double) : 0;
        hipLaunchKernelGGL(proto_loss_bwd_small_kernel, dim3(1 + (d_protos ? d->P : 0)), dim3(PL_THREADS), lds, s, grad_loss, logits, scores,
                           target, protos, fc_w, fc_mask, *d, d_logits, d_scores, d_protos, d_fc_w);
    }
    if (d_occ) {
        const int blocks = ceil_div((long)d->N * d->P, PL_WAVES);
        const float* rownorm = workspace;
        const void* src = d->w_map != 0.0f ? occ : d_occ;  // weight 0: zeros are written, the source is not read
        if (d->map_dtype == PASN_BF16)
            hipLaunchKernelGGL(proto_loss_bwd_map_kernel<__bf16>, dim3(blocks), dim3(PL_THREADS), 0, s, grad_loss, static_cast<const __bf16*>(src),
                               rownorm, *d, pl_vec_ok(src, d_occ, d->S, 2), static_cast<__bf16*>(d_occ));
        else
            hipLaunchKernelGGL(proto_loss_bwd_map_kernel<float>, dim3(blocks), dim3(PL_THREADS), 0, s, grad_loss, static_cast<const float*>(src),
                               rownorm, *d, pl_vec_ok(src, d_occ, d->S, 4), static_cast<float*>(d_occ));
    }
    return check_launch("proto_loss_bwd");
}
