// emd.hip -- approximate earth mover's distance (utils/emd.py: emd_cuda.approxmatch_forward + matchcost_forward from
// PyTorchEMD, an un-vendored third-party extension -- its published algorithm, Fan et al. "A Point Set Generation
// Network", is restated here; call site utils/evaluations.py:45).
//
// Ten annealing levels j = 7 .. -2 with kernel exp(level * |p - q|^2), level = -4^j (0 on the last): each level
//   ratioL[k] = remainL[k] / (1e-9 + sum_l K(k,l) remainR[l])
//   sumr[l]   = remainR[l] * sum_k K(k,l) ratioL[k];  ratioR[l] = min(remainR[l]/(sumr+1e-9), 1) * remainR[l];
//   remainR[l] = max(0, remainR[l] - sumr)
//   match[k,l] += K(k,l) ratioL[k] ratioR[l];   remainL[k] = max(0, remainL[k] - sum_l (that increment))
// and cost = sum_{k,l} match[k,l] * |p_k - q_l|.  The match matrix (n*m floats per cloud pair, 2.7 GB at cfg-2) is
// never stored: the cost is linear in it, so every increment is priced as it is produced.
// One workgroup per cloud pair (the levels are a serial chain), the other cloud tiled through LDS.
//
// The match matrix is determined by the 10 (n + m) ratio values of a cloud pair: emd_kernel<true> keeps them (level i = 7 - j writes
// its ratioL, ratioR into tape[b][i][0 .. n + m) instead of the workspace; same arithmetic, same order, the same cost bits), and
// caspr_emd_bwd_f32 (backward_points.hip) rebuilds every entry from them for the gradient of the cost.
//
// Two forward routes.  "frame" (emd_kernel, caspr_emd_f32 / caspr_emd_tape_f32, the default): one workgroup per frame, whose time does
// not fall with the frame count until the chip is full.  "rows" (caspr_emd_rows_f32, below the frame route's entries; opt-in through
// ops.EMD_ROUTE): the rows of every frame over the grid, 22 ordinary launches in stream order -- the same ratios, tape and gradient bit
// for bit, the cost summed per row and then in a fixed order that depends on n alone.
#include "common.h"

#define EMD_TILE 1024

template <bool TAPE>
__global__ __launch_bounds__(256) void emd_kernel(const float *__restrict__ xyz1, const float *__restrict__ xyz2, int n, int m,
                                                  float *__restrict__ cost, float *__restrict__ ws, float *__restrict__ tape)
{
    __shared__ float buf[EMD_TILE * 4];
    __shared__ float red[256];
    const int i = blockIdx.x, tid = threadIdx.x;
    const float *p1 = xyz1 + (long)i * n * 3, *p2 = xyz2 + (long)i * m * 3;
    float *remainL = ws + (long)i * 2 * (n + m), *remainR = remainL + n, *ratioL = remainR + m, *ratioR = ratioL + n;
    const float multiL = n >= m ? 1.0f : (float)(m / n), multiR = n >= m ? (float)(n / m) : 1.0f;   // integer ratios, as published
    for (int k = tid; k < n; k += 256) remainL[k] = multiL;
    for (int l = tid; l < m; l += 256) remainR[l] = multiR;
    float my_cost = 0.f;
    __syncthreads();
    for (int j = 7; j >= -2; --j) {
        const float level = j == -2 ? 0.0f : -powf(4.0f, (float)j);
        if (TAPE) { ratioL = tape + ((long)i * 10 + (7 - j)) * (n + m); ratioR = ratioL + n; }
        // pass 1: ratioL
        for (int k0 = 0; k0 < n; k0 += 256) {
            const int k = k0 + tid;
            float x1 = 0, y1 = 0, z1 = 0;
            if (k < n) { x1 = p1[k * 3]; y1 = p1[k * 3 + 1]; z1 = p1[k * 3 + 2]; }
            float suml = 1e-9f;
            for (int l0 = 0; l0 < m; l0 += EMD_TILE) {
                const int lend = (m - l0) < EMD_TILE ? (m - l0) : EMD_TILE;
                for (int l = tid; l < lend; l += 256) {
                    buf[l * 4 + 0] = p2[(l0 + l) * 3]; buf[l * 4 + 1] = p2[(l0 + l) * 3 + 1]; buf[l * 4 + 2] = p2[(l0 + l) * 3 + 2];
                    buf[l * 4 + 3] = remainR[l0 + l];
                }
                __syncthreads();
                for (int l = 0; l < lend; ++l) {
                    const float dx = buf[l * 4] - x1, dy = buf[l * 4 + 1] - y1, dz = buf[l * 4 + 2] - z1;
                    suml += expf(level * (dx * dx + dy * dy + dz * dz)) * buf[l * 4 + 3];
                }
                __syncthreads();
            }
            if (k < n) ratioL[k] = remainL[k] / suml;
        }
        __syncthreads();
        // pass 2: ratioR, remainR
        for (int l0 = 0; l0 < m; l0 += 256) {
            const int l = l0 + tid;
            float x2 = 0, y2 = 0, z2 = 0;
            if (l < m) { x2 = p2[l * 3]; y2 = p2[l * 3 + 1]; z2 = p2[l * 3 + 2]; }
            float sumr = 0.f;
            for (int k0 = 0; k0 < n; k0 += EMD_TILE) {
                const int kend = (n - k0) < EMD_TILE ? (n - k0) : EMD_TILE;
                for (int k = tid; k < kend; k += 256) {
                    buf[k * 4 + 0] = p1[(k0 + k) * 3]; buf[k * 4 + 1] = p1[(k0 + k) * 3 + 1]; buf[k * 4 + 2] = p1[(k0 + k) * 3 + 2];
                    buf[k * 4 + 3] = ratioL[k0 + k];
                }
                __syncthreads();
                for (int k = 0; k < kend; ++k) {
                    const float dx = x2 - buf[k * 4], dy = y2 - buf[k * 4 + 1], dz = z2 - buf[k * 4 + 2];
                    sumr += expf(level * (dx * dx + dy * dy + dz * dz)) * buf[k * 4 + 3];
                }
                __syncthreads();
            }
            if (l < m) {
                const float rr = remainR[l];
                sumr *= rr;
                const float consumption = fminf(rr / (sumr + 1e-9f), 1.0f);
                ratioR[l] = consumption * rr;
                remainR[l] = fmaxf(0.0f, rr - sumr);
            }
        }
        __syncthreads();
        // pass 3: the match increment, priced immediately; remainL
        for (int k0 = 0; k0 < n; k0 += 256) {
            const int k = k0 + tid;
            float x1 = 0, y1 = 0, z1 = 0, rl = 0;
            if (k < n) { x1 = p1[k * 3]; y1 = p1[k * 3 + 1]; z1 = p1[k * 3 + 2]; rl = ratioL[k]; }
            float suml = 0.f;
            for (int l0 = 0; l0 < m; l0 += EMD_TILE) {
                const int lend = (m - l0) < EMD_TILE ? (m - l0) : EMD_TILE;
                for (int l = tid; l < lend; l += 256) {
                    buf[l * 4 + 0] = p2[(l0 + l) * 3]; buf[l * 4 + 1] = p2[(l0 + l) * 3 + 1]; buf[l * 4 + 2] = p2[(l0 + l) * 3 + 2];
                    buf[l * 4 + 3] = ratioR[l0 + l];
                }
                __syncthreads();
                if (k < n) {
                    for (int l = 0; l < lend; ++l) {
                        const float dx = buf[l * 4] - x1, dy = buf[l * 4 + 1] - y1, dz = buf[l * 4 + 2] - z1;
                        const float d2 = dx * dx + dy * dy + dz * dz;
                        const float v = expf(level * d2) * rl * buf[l * 4 + 3];
                        suml += v;
                        my_cost += v * sqrtf(d2);
                    }
                }
                __syncthreads();
            }
            if (k < n) remainL[k] = fmaxf(0.0f, remainL[k] - suml);
        }
        __syncthreads();
    }
    red[tid] = my_cost;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) cost[i] = red[0];
}

extern "C" long caspr_emd_ws_bytes(int B, int n, int m) { return (long)B * 2 * (n + m) * 4 + 256; }

extern "C" int caspr_emd_f32(const float *xyz1, const float *xyz2, int B, int n, int m, float *cost, void *ws, long ws_bytes,
                             void *stream)
{
    CASPR_REQUIRE(xyz1 && xyz2 && cost && ws && B > 0 && n > 0 && m > 0, "emd: bad arguments");
    CASPR_REQUIRE(ws_bytes >= caspr_emd_ws_bytes(B, n, m), "emd: workspace too small");
    emd_kernel<false><<<dim3(B), dim3(256), 0, (hipStream_t)stream>>>(xyz1, xyz2, n, m, cost, (float *)ws, nullptr);
    CASPR_CHECK_LAUNCH("emd");
    return CASPR_OK;
}

extern "C" long caspr_emd_tape_bytes(int B, int n, int m) { return (long)B * 10 * (n + m) * 4; }

extern "C" int caspr_emd_tape_f32(const float *xyz1, const float *xyz2, int B, int n, int m, float *cost, float *tape, void *ws,
                                  long ws_bytes, void *stream)
{
    CASPR_REQUIRE(xyz1 && xyz2 && cost && tape && ws && B > 0 && n > 0 && m > 0, "emd_tape: bad arguments");
    CASPR_REQUIRE(ws_bytes >= caspr_emd_ws_bytes(B, n, m), "emd_tape: workspace too small");
    emd_kernel<true><<<dim3(B), dim3(256), 0, (hipStream_t)stream>>>(xyz1, xyz2, n, m, cost, (float *)ws, tape);
    CASPR_CHECK_LAUNCH("emd_tape");
    return CASPR_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// The "rows" route (caspr_emd_rows_f32): the same ten levels with the ROWS of every frame spread over the grid instead of one workgroup
// per frame.  A row's sum (ratioL[k] over l, ratioR[l] over k, the match increment of row k over l) is a sequential f32 chain and the
// rows are independent, so every per-pair expression below is emd_kernel's, operand for operand, and every ratio is its ratio bit for
// bit; only the cost is added in another order (below).  No workgroup waits for another: the order between passes is the stream's.
// 22 ordinary launches on the caller's stream, each with grid (row blocks of EMD_ROWS, B):
//   emd_rows_ca_kernel<false, true>   A of level 7:  remainL = multiL, ratioL_7[k] = remainL[k] / (1e-9 + sum_l K remainR[l])  (remainR = multiR)
//   for j = 7 .. -1:  emd_rows_b_kernel          B of level j:  ratioR_j, remainR                          (one thread per row l, k ascending)
//                     emd_rows_ca_kernel<true, true>   C of level j and A of level j - 1 in ONE sweep over l (the same rows k, the same
//                                                tile): v = K_j ratioL_j[k] ratioR_j[l]; suml += v; rowcost[k] += v sqrtf(d2);
//                                                remainL[k] = max(0, remainL[k] - suml); then ratioL_{j-1}[k] from the new remainL[k]
//   emd_rows_b_kernel, emd_rows_ca_kernel<true, false>   B and C of the last level (j = -2, level 0)
//   emd_rows_cost_kernel              cost[b] = sum_k rowcost[k]
// rowcost[k] is ONE f32 accumulator per row carried through the ten levels (l ascending inside a level, levels 7 .. -2), where emd_kernel
// carries one per lane through all of the lane's rows.  The final order is a function of n alone: thread t of 256 adds rowcost[t],
// rowcost[t + 256], ... ascending, then the 256 partial sums meet in the binary tree emd_kernel ends with (t += t + w, w = 128 .. 1).
// A frame's result depends on nothing but the frame: not on B, its place in the batch or the device.
// Workspace per frame: remainL (n) | remainR (m) | rowcost (n) | ratioL (n) | ratioR (m); the last two are used when there is no tape.
#define EMD_ROWS 256

struct EmdRowsFrame {
    const float *p1, *p2;
    float *remainL, *remainR, *rowcost, *ratio;   // ratio: level 0's ratioL of this frame (tape) or the workspace's single pair
    long level_stride;                            // n + m with a tape, 0 without
};

__device__ __forceinline__ EmdRowsFrame emd_rows_frame(const float *xyz1, const float *xyz2, int n, int m, float *ws, float *tape)
{
    const long b = blockIdx.y, nm = (long)n + m;
    EmdRowsFrame f;
    f.p1 = xyz1 + b * n * 3;
    f.p2 = xyz2 + b * m * 3;
    f.remainL = ws + b * (nm * 2 + n);
    f.remainR = f.remainL + n;
    f.rowcost = f.remainR + m;
    f.ratio = tape ? tape + b * 10 * nm : f.rowcost + n;
    f.level_stride = tape ? nm : 0;
    return f;
}

// pass C of level j (HAS_C) and pass A of level j - 1 (HAS_A), one thread per row k of cloud 1
template <bool HAS_C, bool HAS_A>
__global__ __launch_bounds__(EMD_ROWS) void emd_rows_ca_kernel(const float *__restrict__ xyz1, const float *__restrict__ xyz2, int n, int m, int j,
                                                               float *ws, float *tape)
{
    __shared__ float buf[EMD_TILE * 4];    // x, y, z of cloud 2 and ratioR of level j
    __shared__ float wa[EMD_TILE];         // remainR, the weight of pass A
    const EmdRowsFrame f = emd_rows_frame(xyz1, xyz2, n, m, ws, tape);
    const float *p1 = f.p1, *p2 = f.p2;
    const int tid = threadIdx.x, k = blockIdx.x * EMD_ROWS + tid, ja = j - 1;
    const float multiL = n >= m ? 1.0f : (float)(m / n), multiR = n >= m ? (float)(n / m) : 1.0f;   // integer ratios, as published
    const float level = j == -2 ? 0.0f : -powf(4.0f, (float)j), level_a = ja == -2 ? 0.0f : -powf(4.0f, (float)ja);
    const float *ratioL = f.ratio + (7 - j) * f.level_stride, *ratioR = ratioL + n;
    float *ratioL_a = f.ratio + (7 - ja) * f.level_stride;
    float x1 = 0, y1 = 0, z1 = 0, rl = 0, rem = multiL, rc = 0.f;
    if (k < n) {
        x1 = p1[k * 3]; y1 = p1[k * 3 + 1]; z1 = p1[k * 3 + 2];
        if (HAS_C) { rl = ratioL[k]; rem = f.remainL[k]; if (j != 7) rc = f.rowcost[k]; }
    }
    float suml = 0.f, suml_a = 1e-9f;
    for (int l0 = 0; l0 < m; l0 += EMD_TILE) {
        const int lend = (m - l0) < EMD_TILE ? (m - l0) : EMD_TILE;
        for (int l = tid; l < lend; l += EMD_ROWS) {
            buf[l * 4 + 0] = p2[(l0 + l) * 3]; buf[l * 4 + 1] = p2[(l0 + l) * 3 + 1]; buf[l * 4 + 2] = p2[(l0 + l) * 3 + 2];
            if (HAS_C) buf[l * 4 + 3] = ratioR[l0 + l];
            if (HAS_A) wa[l] = HAS_C ? f.remainR[l0 + l] : multiR;
        }
        __syncthreads();
        if (k < n) {
            for (int l = 0; l < lend; ++l) {
                const float dx = buf[l * 4] - x1, dy = buf[l * 4 + 1] - y1, dz = buf[l * 4 + 2] - z1;
                const float d2 = dx * dx + dy * dy + dz * dz;
                if (HAS_C) {
                    const float v = expf(level * d2) * rl * buf[l * 4 + 3];
                    suml += v;
                    rc += v * sqrtf(d2);
                }
                if (HAS_A) suml_a += expf(level_a * d2) * wa[l];
            }
        }
        __syncthreads();
    }
    if (k < n) {
        if (HAS_C) { rem = fmaxf(0.0f, rem - suml); f.rowcost[k] = rc; }
        if (HAS_A) { f.remainL[k] = rem; ratioL_a[k] = rem / suml_a; }
    }
}

// pass B of level j, one thread per row l of cloud 2
__global__ __launch_bounds__(EMD_ROWS) void emd_rows_b_kernel(const float *__restrict__ xyz1, const float *__restrict__ xyz2, int n, int m, int j,
                                                              float *ws, float *tape)
{
    __shared__ float buf[EMD_TILE * 4];    // x, y, z of cloud 1 and ratioL of level j
    const EmdRowsFrame f = emd_rows_frame(xyz1, xyz2, n, m, ws, tape);
    const float *p1 = f.p1, *p2 = f.p2;
    const int tid = threadIdx.x, l = blockIdx.x * EMD_ROWS + tid;
    const float multiR = n >= m ? (float)(n / m) : 1.0f;
    const float level = j == -2 ? 0.0f : -powf(4.0f, (float)j);
    const float *ratioL = f.ratio + (7 - j) * f.level_stride;
    float *ratioR = f.ratio + (7 - j) * f.level_stride + n;
    float x2 = 0, y2 = 0, z2 = 0;
    if (l < m) { x2 = p2[l * 3]; y2 = p2[l * 3 + 1]; z2 = p2[l * 3 + 2]; }
    float sumr = 0.f;
    for (int k0 = 0; k0 < n; k0 += EMD_TILE) {
        const int kend = (n - k0) < EMD_TILE ? (n - k0) : EMD_TILE;
        for (int k = tid; k < kend; k += EMD_ROWS) {
            buf[k * 4 + 0] = p1[(k0 + k) * 3]; buf[k * 4 + 1] = p1[(k0 + k) * 3 + 1]; buf[k * 4 + 2] = p1[(k0 + k) * 3 + 2];
            buf[k * 4 + 3] = ratioL[k0 + k];
        }
        __syncthreads();
        if (l < m) {
            for (int k = 0; k < kend; ++k) {
                const float dx = x2 - buf[k * 4], dy = y2 - buf[k * 4 + 1], dz = z2 - buf[k * 4 + 2];
                sumr += expf(level * (dx * dx + dy * dy + dz * dz)) * buf[k * 4 + 3];
            }
        }
        __syncthreads();
    }
    if (l < m) {
        const float rr = j == 7 ? multiR : f.remainR[l];   // level 7 starts from the full weight: nothing has written remainR yet
        sumr *= rr;
        const float consumption = fminf(rr / (sumr + 1e-9f), 1.0f);
        ratioR[l] = consumption * rr;
        f.remainR[l] = fmaxf(0.0f, rr - sumr);
    }
}

__global__ __launch_bounds__(256) void emd_rows_cost_kernel(const float *__restrict__ ws, int n, int m, float *__restrict__ cost)
{
    __shared__ float red[256];
    const long b = blockIdx.y;
    const int tid = threadIdx.x;
    const float *rowcost = ws + b * (((long)n + m) * 2 + n) + n + m;
    float s = 0.f;
    for (int k = tid; k < n; k += 256) s += rowcost[k];
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) cost[b] = red[0];
}

extern "C" long caspr_emd_rows_ws_bytes(int B, int n, int m) { return (long)B * (3L * n + 2L * m) * 4 + 256; }

extern "C" int caspr_emd_rows_f32(const float *xyz1, const float *xyz2, int B, int n, int m, float *cost, float *tape, void *ws,
                                  long ws_bytes, void *stream)
{
    CASPR_REQUIRE(xyz1 && xyz2 && cost && ws && B > 0 && n > 0 && m > 0, "emd_rows: bad arguments");
    CASPR_REQUIRE(B <= 65535, "emd_rows: B=%d: the cloud index is grid.y, B <= 65535", B);
    CASPR_REQUIRE(ws_bytes >= caspr_emd_rows_ws_bytes(B, n, m), "emd_rows: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const dim3 gk(ceil_div(n, EMD_ROWS), B), gl(ceil_div(m, EMD_ROWS), B), blk(EMD_ROWS);
    float *w = (float *)ws;
    emd_rows_ca_kernel<false, true><<<gk, blk, 0, st>>>(xyz1, xyz2, n, m, 8, w, tape);
    for (int j = 7; j >= -2; --j) {
        emd_rows_b_kernel<<<gl, blk, 0, st>>>(xyz1, xyz2, n, m, j, w, tape);
        if (j > -2) emd_rows_ca_kernel<true, true><<<gk, blk, 0, st>>>(xyz1, xyz2, n, m, j, w, tape);
        else emd_rows_ca_kernel<true, false><<<gk, blk, 0, st>>>(xyz1, xyz2, n, m, j, w, tape);
    }
    emd_rows_cost_kernel<<<dim3(1, B), dim3(256), 0, st>>>(w, n, m, cost);
    CASPR_CHECK_LAUNCH("emd_rows");
    return CASPR_OK;
}
