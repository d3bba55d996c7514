// fcos_loss.hip -- the training step of CondInst's box head (include/boxinst/boxinst_hip_fcos.h): FCOS target assignment, sigmoid
// focal loss, IoU / GIoU loss and centerness loss with their finished gradients, and the backward rescale.  gfx950 only.
//
//   fcos_targets_kernel         one workgroup of 256 per (level, image, tile of 256 locations), one thread per location.  The image's
//                               boxes pass through LDS in chunks of BXI_FCOS_GT_CHUNK (every lane reads the same box: a broadcast).
//                               Writes every target row and the workgroup's partial (positives, centerness sum in fp64, bad-label flag).
//   fcos_focal_kernel<G2>       flat over the [B][C][HW] logits of a level, four consecutive elements per thread (one 16-byte load and
//                               store where the pointers allow it, four scalar ones elsewhere and on the level's tail -- the same
//                               element-to-thread map either way, so the sums do not depend on alignment).  G2: gamma == 2.
//   fcos_pos_kernel             the grid of fcos_targets_kernel: IoU / GIoU and centerness loss of the positives and the gradient
//                               w.r.t. the four distances and the centerness logit; zeros on every other location.
//   fcos_finish_kernel          one workgroup: adds the partials of the workgroups in a fixed order (thread t takes partials t, t + 256,
//                               ...; then the wave totals, then the four waves; fp64 accumulators), writes
//                               stats / status or the three losses.
//   fcos_rescale_kernel         out = unit * upstream[k], flat over every map of every level.
// No kernel keeps an array that is indexed at run time in registers; none uses scratch (profiles/NOTES.md, round 11).
#include "focal_device.hpp"

// (fp contraction is off for the whole file: focal_device.hpp says why)
#pragma clang fp contract(off)

namespace bxi {
namespace {

constexpr int kChunk = BXI_FCOS_GT_CHUNK;
constexpr float kInf = 1e8f;                 // condinst_head.py:16

struct Ranges { float lo[kMaxL], hi[kMaxL], radius[kMaxL]; };   // radius = (float)(stride * center_sample_radius)
struct Maps {
    const float* cls[kMaxL]; const float* bbox[kMaxL]; const float* ctr[kMaxL];
    float* gcls[kMaxL]; float* gbbox[kMaxL]; float* gctr[kMaxL];
};
__device__ __forceinline__ void locate(const LocGrid& g, int& l, int& b, int& yx) {
    const int blk = blockIdx.x;
    l = 0;
    while (l + 1 < g.n && blk >= g.blk_first[l + 1]) ++l;
    const int r = blk - g.blk_first[l];
    b = r / g.tiles[l];
    yx = (r - b * g.tiles[l]) * kLocTile + threadIdx.x;
}

// ---- targets --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLocTile) void fcos_targets_kernel(LocGrid g, Ranges rg, GtOffsets off, int center_sampling, int norm_on_bbox,
                                                                int num_classes, const float* __restrict__ gt_boxes,
                                                                const int64_t* __restrict__ gt_labels, int64_t* __restrict__ labels,
                                                                float* __restrict__ bbox_targets, int64_t* __restrict__ gt_inds,
                                                                float* __restrict__ points, int64_t* __restrict__ level_inds,
                                                                int64_t* __restrict__ img_inds, float* __restrict__ ctr_targets,
                                                                int32_t* __restrict__ partials) {
    __shared__ float sx1[kChunk], sy1[kChunk], sx2[kChunk], sy2[kChunk], sarea[kChunk];
    __shared__ int slab[kChunk];
    __shared__ int s_bad;
    __shared__ double s4d[4];
    __shared__ int s4i[4];
    int l, b, yx;
    locate(g, l, b, yx);
    const int tid = threadIdx.x;
    const int hw = g.H[l] * g.W[l];
    const bool live = yx < hw;
    const float st = (float)g.stride[l];
    const int y = live ? yx / g.W[l] : 0, x = live ? yx - y * g.W[l] : 0;
    const float xs = f_mul((float)x + 0.5f, st), ys = f_mul((float)y + 0.5f, st);
    const float lo = rg.lo[l], hi = rg.hi[l], rad = rg.radius[l];
    const int g0 = off.v[b], n_gt = off.v[b + 1] - g0;
    if (tid == 0) s_bad = 0;

    float best = kInf;
    int best_i = 0, best_lab = -1;
    float bl = 0.f, bt = 0.f, br = 0.f, bb = 0.f;
    for (int c0 = 0; c0 < n_gt; c0 += kChunk) {
        const int nc = min(kChunk, n_gt - c0);
        __syncthreads();                                   // the previous chunk has been read (and s_bad = 0 is in place)
        if (tid < nc) {
            const float* p = gt_boxes + 4 * (size_t)(g0 + c0 + tid);
            const float x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3];
            sx1[tid] = x1; sy1[tid] = y1; sx2[tid] = x2; sy2[tid] = y2;
            sarea[tid] = f_mul(f_sub(x2, x1), f_sub(y2, y1));
            const int64_t lab = gt_labels[g0 + c0 + tid];
            const bool ok = lab >= 0 && lab < num_classes;
            slab[tid] = ok ? (int)lab : -1;
            if (!ok) s_bad = 1;
        }
        __syncthreads();
        for (int k = 0; k < nc; ++k) {
            const float x1 = sx1[k], y1 = sy1[k], x2 = sx2[k], y2 = sy2[k];
            const float dl = f_sub(xs, x1), dr = f_sub(x2, xs), dt = f_sub(ys, y1), db = f_sub(y2, ys);
            bool inside;
            if (center_sampling) {
                const float cx = f_div(f_add(x1, x2), 2.f), cy = f_div(f_add(y1, y2), 2.f);
                const float xmin = f_sub(cx, rad), ymin = f_sub(cy, rad), xmax = f_add(cx, rad), ymax = f_add(cy, rad);
                const float c_x1 = xmin > x1 ? xmin : x1, c_y1 = ymin > y1 ? ymin : y1;
                const float c_x2 = xmax > x2 ? x2 : xmax, c_y2 = ymax > y2 ? y2 : ymax;
                const float m = fminf(fminf(f_sub(xs, c_x1), f_sub(ys, c_y1)), fminf(f_sub(c_x2, xs), f_sub(c_y2, ys)));
                inside = m > 0.f;
            } else {
                inside = fminf(fminf(dl, dt), fminf(dr, db)) > 0.f;
            }
            const float mx = fmaxf(fmaxf(dl, dt), fmaxf(dr, db));
            const bool in_range = mx >= lo && mx <= hi;
            const float a = (inside && in_range) ? sarea[k] : kInf;
            // box 0 starts the minimum whatever it holds (a row of sentinels has its arg-min there); later boxes need a smaller value
            if (c0 + k == 0 || a < best) {
                best = a;
                best_i = c0 + k;
                best_lab = slab[k];
                bl = dl; bt = dt; br = dr; bb = db;
            }
        }
    }
    __syncthreads();
    const bool pos = live && n_gt > 0 && best != kInf && best_lab >= 0;
    float ct = 0.f;
    if (live) {
        if (n_gt > 0 && norm_on_bbox) {
            bl = f_div(bl, st); bt = f_div(bt, st); br = f_div(br, st); bb = f_div(bb, st);
        }
        if (pos) {
            const float lr = f_div(fminf(bl, br), fmaxf(bl, br)), tb = f_div(fminf(bt, bb), fmaxf(bt, bb));
            ct = sqrtf(f_mul(lr, tb));
        }
        const size_t n = (size_t)g.B * g.first[l] + (size_t)b * hw + yx;
        labels[n] = pos ? best_lab : num_classes;
        gt_inds[n] = pos ? (int64_t)(g0 + best_i) : -1;
        bbox_targets[4 * n + 0] = bl; bbox_targets[4 * n + 1] = bt; bbox_targets[4 * n + 2] = br; bbox_targets[4 * n + 3] = bb;
        points[2 * n + 0] = xs; points[2 * n + 1] = ys;
        level_inds[n] = l;
        img_inds[n] = b;
        ctr_targets[n] = ct;
    }
    const int npos = block_sum_4w_i32(pos ? 1 : 0, s4i);
    const double csum = block_sum_4w_f64((double)ct, s4d);
    if (tid == 0) {
        int32_t* p = partials + 4 * (size_t)blockIdx.x;
        const long long cbits = __double_as_longlong(csum);     // the centerness sum stays fp64 until the one final rounding
        p[0] = npos;
        p[1] = (int32_t)cbits;
        p[2] = (int32_t)(cbits >> 32);
        p[3] = s_bad;
    }
}

// mode 0: stats [2] and status from the targets' partials; mode 1: losses [3] from the loss kernels' partials (three floats each)
__global__ __launch_bounds__(256) void fcos_finish_kernel(const int32_t* __restrict__ partials, int n_blocks, int mode, float* __restrict__ out,
                                                          int32_t* __restrict__ status) {
    __shared__ double s4d[4];
    __shared__ int s4i[4];
    const int tid = threadIdx.x;
    if (mode == 0) {
        int np = 0, bad = 0;
        double cs = 0.0;
        for (int i = tid; i < n_blocks; i += 256) {
            np += partials[4 * (size_t)i];
            cs += __longlong_as_double(((long long)partials[4 * (size_t)i + 2] << 32) | (unsigned int)partials[4 * (size_t)i + 1]);
            bad |= partials[4 * (size_t)i + 3];
        }
        np = block_sum_4w_i32(np, s4i);
        bad = block_sum_4w_i32(bad ? 1 : 0, s4i);
        cs = block_sum_4w_f64(cs, s4d);
        if (tid == 0) {
            out[0] = (float)np;
            out[1] = (float)cs;
            status[0] = bad ? BXI_FCOS_STATUS_BAD_LABEL : 0;
        }
        return;
    }
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int i = tid; i < n_blocks; i += 256) {
        a0 += (double)__int_as_float(partials[4 * (size_t)i]);
        a1 += (double)__int_as_float(partials[4 * (size_t)i + 1]);
        a2 += (double)__int_as_float(partials[4 * (size_t)i + 2]);
    }
    a0 = block_sum_4w_f64(a0, s4d);
    a1 = block_sum_4w_f64(a1, s4d);
    a2 = block_sum_4w_f64(a2, s4d);
    if (tid == 0) {
        out[0] = (float)a0;
        out[1] = (float)a1;
        out[2] = (float)a2;
    }
}

// ---- focal loss -----------------------------------------------------------------------------------------------------------
template <bool G2>
__global__ __launch_bounds__(256) void fcos_focal_kernel(Maps m, LocGrid g, FlatGrid f, int C, const int64_t* __restrict__ labels,
                                                         const float* __restrict__ norm, float gamma, float alpha, float lw,
                                                         int32_t* __restrict__ partials, int part_first) {
    __shared__ double s4d[4];
    const int blk = blockIdx.x, tid = threadIdx.x;
    int l = 0;
    while (l + 1 < f.n && blk >= f.blk_first[l + 1]) ++l;
    const int count = f.count[l];
    const int e0 = (blk - f.blk_first[l]) * kElemTile + tid * 4;
    const int hw = g.H[l] * g.W[l];
    const float* __restrict__ src = m.cls[l];
    float* __restrict__ dst = m.gcls[l];
    const float denom = fmaxf(norm[0], 1.f) + FLT_EPSILON;
    const float scale = lw / denom;
    const double tot = focal_tile<G2>(src, dst, count, e0, hw, C, (size_t)g.B * g.first[l], labels, gamma, alpha, scale, s4d);
    if (tid == 0) {
        int32_t* p = partials + 4 * (size_t)(part_first + blk);
        p[0] = __float_as_int((float)(tot * (double)scale));
        p[1] = 0;
        p[2] = 0;
        p[3] = 0;
    }
}

// ---- IoU / GIoU and centerness loss of the positives ----------------------------------------------------------------------
// gradient share of `a` in max(a, b) / min(a, b) of two tensors (torch: halves at equality)
__device__ __forceinline__ float share_max(float a, float b) { return a > b ? 1.f : (a == b ? 0.5f : 0.f); }
__device__ __forceinline__ float share_min(float a, float b) { return a < b ? 1.f : (a == b ? 0.5f : 0.f); }

__global__ __launch_bounds__(kLocTile) void fcos_pos_kernel(Maps m, LocGrid g, int C, const int64_t* __restrict__ labels,
                                                            const float* __restrict__ bbox_targets, const float* __restrict__ ctr_targets,
                                                            const float* __restrict__ norm, float lw_bbox, float lw_ctr, int kind, float eps,
                                                            int32_t* __restrict__ partials, int part_first) {
    __shared__ double s4d[4];
    int l, b, yx;
    locate(g, l, b, yx);
    const int hw = g.H[l] * g.W[l];
    const bool live = yx < hw;
    float loss_b = 0.f, loss_c = 0.f;
    const float scale_b = lw_bbox / (fmaxf(norm[1], 1e-6f) + FLT_EPSILON);
    const float scale_c = lw_ctr / (fmaxf(norm[0], 1.f) + FLT_EPSILON);
    if (live) {
        const size_t n = (size_t)g.B * g.first[l] + (size_t)b * hw + yx;
        const int64_t lab = labels[n];
        float gd[4] = {0.f, 0.f, 0.f, 0.f}, gc = 0.f;
        if (lab >= 0 && lab < C) {
            const float st = (float)g.stride[l];
            const int y = yx / g.W[l], x = yx - y * g.W[l];
            const float px = f_mul((float)x + 0.5f, st), py = f_mul((float)y + 0.5f, st);
            const float* d = m.bbox[l] + (size_t)b * 4 * hw + yx;
            const float* tg = bbox_targets + 4 * n;
            const float w_i = ctr_targets[n];
            // distance2bbox of both (transforms.py:153-156)
            const float px1 = f_sub(px, d[0]), py1 = f_sub(py, d[hw]), px2 = f_add(px, d[2 * hw]), py2 = f_add(py, d[3 * hw]);
            const float tx1 = f_sub(px, tg[0]), ty1 = f_sub(py, tg[1]), tx2 = f_add(px, tg[2]), ty2 = f_add(py, tg[3]);
            // products and sums as single fp32 operations: with prediction == target, overlap, union and the enclosing area are then
            // the same number, as in torch, and IoU = GIoU = 1 exactly (contracted into an FMA they would differ by a rounding)
            const float w1 = f_sub(px2, px1), h1 = f_sub(py2, py1);
            const float area1 = f_mul(w1, h1), area2 = f_mul(f_sub(tx2, tx1), f_sub(ty2, ty1));
            const float wx = f_sub(fminf(px2, tx2), fmaxf(px1, tx1)), hy = f_sub(fminf(py2, ty2), fmaxf(py1, ty1));
            const float w = wx >= 0.f ? wx : 0.f, h = hy >= 0.f ? hy : 0.f;
            const float overlap = f_mul(w, h);
            const float union_ = f_sub(f_add(area1, area2), overlap);
            const float eps_u = kind == BXI_FCOS_BBOX_GIOU ? eps : 1e-6f;          // bbox_overlaps' own default inside iou_loss
            const float uc = fmaxf(union_, eps_u);
            const float iou = f_div(overlap, uc);
            float li, d_overlap, d_uc, d_ec = 0.f;
            float ewx = 0.f, ehy = 0.f, ew = 0.f, eh = 0.f, earea = 0.f;
            if (kind == BXI_FCOS_BBOX_GIOU) {
                ewx = f_sub(fmaxf(px2, tx2), fminf(px1, tx1));
                ehy = f_sub(fmaxf(py2, ty2), fminf(py1, ty1));
                ew = ewx >= 0.f ? ewx : 0.f;
                eh = ehy >= 0.f ? ehy : 0.f;
                earea = f_mul(ew, eh);
                const float ec = fmaxf(earea, eps);
                li = f_sub(1.f, f_sub(iou, f_div(f_sub(ec, uc), ec)));
                // loss = 1 - iou + 1 - uc / ec
                d_overlap = -1.f / uc;
                d_uc = overlap / (uc * uc) - 1.f / ec;
                d_ec = uc / (ec * ec);
            } else {
                const float ic = fmaxf(iou, eps);
                const float pass = iou >= eps ? 1.f : 0.f;                            // clamp(min=eps)
                float d_iou;
                if (kind == BXI_FCOS_BBOX_IOU_LOG) { li = -logf(ic); d_iou = -1.f / ic; }
                else if (kind == BXI_FCOS_BBOX_IOU_LINEAR) { li = 1.f - ic; d_iou = -1.f; }
                else { li = 1.f - ic * ic; d_iou = -2.f * ic; }
                d_iou *= pass;
                d_overlap = d_iou / uc;
                d_uc = -d_iou * overlap / (uc * uc);
            }
            const float d_union = d_uc * share_max(union_, eps_u);
            const float d_area1 = d_union;
            d_overlap -= d_union;
            const float d_wx = wx >= 0.f ? d_overlap * h : 0.f, d_hy = hy >= 0.f ? d_overlap * w : 0.f;
            // lt = max(p1, t1), rb = min(p2, t2); wx = rb - lt
            float d_px1 = -d_wx * share_max(px1, tx1) - d_area1 * h1;
            float d_px2 = d_wx * share_min(px2, tx2) + d_area1 * h1;
            float d_py1 = -d_hy * share_max(py1, ty1) - d_area1 * w1;
            float d_py2 = d_hy * share_min(py2, ty2) + d_area1 * w1;
            if (kind == BXI_FCOS_BBOX_GIOU) {
                const float d_earea = d_ec * share_max(earea, eps);
                const float d_ewx = ewx >= 0.f ? d_earea * eh : 0.f, d_ehy = ehy >= 0.f ? d_earea * ew : 0.f;
                d_px2 += d_ewx * share_max(px2, tx2);
                d_px1 -= d_ewx * share_min(px1, tx1);
                d_py2 += d_ehy * share_max(py2, ty2);
                d_py1 -= d_ehy * share_min(py1, ty1);
            }
            const float s = scale_b * w_i;
            gd[0] = -d_px1 * s; gd[1] = -d_py1 * s; gd[2] = d_px2 * s; gd[3] = d_py2 * s;
            loss_b = li * w_i;
            // centerness: BCE with logits against the target
            const float xc = m.ctr[l][(size_t)b * hw + yx];
            const float e = expf(-fabsf(xc));
            const float inv = 1.f / (1.f + e);
            const float sg = xc >= 0.f ? inv : e * inv;
            loss_c = fmaxf(xc, 0.f) - xc * w_i + log1pf(e);
            gc = (sg - w_i) * scale_c;
        }
        float* gb = m.gbbox[l] + (size_t)b * 4 * hw + yx;
        gb[0] = gd[0]; gb[hw] = gd[1]; gb[2 * hw] = gd[2]; gb[3 * hw] = gd[3];
        m.gctr[l][(size_t)b * hw + yx] = gc;
    }
    const double tb = block_sum_4w_f64((double)loss_b, s4d);
    const double tc = block_sum_4w_f64((double)loss_c, s4d);
    if (threadIdx.x == 0) {
        int32_t* p = partials + 4 * (size_t)(part_first + blockIdx.x);
        p[0] = 0;
        p[1] = __float_as_int((float)(tb * (double)scale_b));
        p[2] = __float_as_int((float)(tc * (double)scale_c));
        p[3] = 0;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------
int grid_of(const bxi_fcos_level* levels, int n_levels, int B, LocGrid& g) {
    if (n_levels < 1 || n_levels > kMaxL) return BXI_ERR_BAD_SHAPE;
    if (!levels) return BXI_ERR_NULL_POINTER;
    int H[kMaxL], W[kMaxL], S[kMaxL];
    for (int l = 0; l < n_levels; ++l) { H[l] = levels[l].H; W[l] = levels[l].W; S[l] = levels[l].stride; }
    return make_grid(H, W, S, n_levels, B, g);
}

}  // namespace
}  // namespace bxi

using namespace bxi;

extern "C" size_t bxi_fcos_workspace_bytes(const bxi_fcos_level* levels_host, int n_levels, int B, int C) {
    LocGrid g;
    if (B < 1 || C < 1 || grid_of(levels_host, n_levels, B, g) != BXI_OK) return 0;
    FlatGrid f;
    const int chan[1] = {C};
    const int64_t fb = make_flat(g, chan, 1, f);
    if (fb < 0) return 0;
    return 16 * (size_t)(fb + g.blk_first[g.n]);
}

extern "C" int bxi_fcos_targets_f32(const bxi_fcos_level* levels_host, int n_levels, int B, const float* regress_ranges_host,
                                    int center_sampling, double center_sample_radius, int norm_on_bbox, int num_classes,
                                    const float* gt_boxes, const int64_t* gt_labels, const int* gt_offsets_host, int64_t* labels,
                                    float* bbox_targets, int64_t* gt_inds, float* points, int64_t* level_inds, int64_t* img_inds,
                                    float* ctr_targets, float* stats, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    LocGrid g;
    if (int rc = grid_of(levels_host, n_levels, B, g)) return rc;
    if (num_classes < 1) return BXI_ERR_BAD_SHAPE;
    if (B == 0) return BXI_OK;
    if (!regress_ranges_host || !gt_offsets_host) return BXI_ERR_NULL_POINTER;
    GtOffsets off;
    if (int rc = read_offsets(gt_offsets_host, B, off)) return rc;
    if (!fits_i32((int64_t)off.v[B] * 4)) return BXI_ERR_BAD_SHAPE;
    Ranges rg;
    if (center_sampling && !(center_sample_radius >= 0.0)) return BXI_ERR_BAD_ARGUMENT;
    for (int l = 0; l < kMaxL; ++l) {
        rg.lo[l] = l < n_levels ? regress_ranges_host[2 * l] : 0.f;
        rg.hi[l] = l < n_levels ? regress_ranges_host[2 * l + 1] : 0.f;
        rg.radius[l] = center_sampling ? (float)((double)g.stride[l] * center_sample_radius) : 0.f;    // python: stride * radius, then fp32
        if (rg.lo[l] != rg.lo[l] || rg.hi[l] != rg.hi[l]) return BXI_ERR_BAD_ARGUMENT;
    }
    if (!labels || !bbox_targets || !gt_inds || !points || !level_inds || !img_inds || !ctr_targets || !stats || !status ||
        (off.v[B] > 0 && (!gt_boxes || !gt_labels)))
        return BXI_ERR_NULL_POINTER;
    const int n_blocks = g.blk_first[g.n];
    if (!workspace_ok(workspace, workspace_bytes, 16 * (size_t)n_blocks, 4)) return BXI_ERR_WORKSPACE;
    hipStream_t s = as_stream(stream);
    int32_t* part = static_cast<int32_t*>(workspace);
    BXI_LAUNCH("fcos_targets", s, fcos_targets_kernel, dim3((unsigned)n_blocks), dim3(kLocTile), 0, s, g, rg, off, center_sampling ? 1 : 0,
               norm_on_bbox ? 1 : 0, num_classes, gt_boxes, gt_labels, labels, bbox_targets, gt_inds, points, level_inds, img_inds, ctr_targets,
               part);
    if (int rc = check_launch()) return rc;
    BXI_LAUNCH("fcos_targets_finish", s, fcos_finish_kernel, dim3(1), dim3(256), 0, s, part, n_blocks, 0, stats, status);
    return check_launch();
}

extern "C" int bxi_fcos_loss_f32(const bxi_det_level* levels_host, int n_levels, int B, int C, const int64_t* labels,
                                 const float* bbox_targets, const float* ctr_targets, const float* norm, float gamma, float alpha,
                                 float loss_weight_cls, float loss_weight_bbox, float loss_weight_ctr, int bbox_loss_kind, float eps,
                                 const bxi_fcos_grads* grads_host, float* losses, void* workspace, size_t workspace_bytes, void* stream) {
    if (n_levels < 1 || n_levels > kMaxL || C < 1) return BXI_ERR_BAD_SHAPE;
    if (!levels_host) return BXI_ERR_NULL_POINTER;
    int H[kMaxL], W[kMaxL], S[kMaxL];
    for (int l = 0; l < n_levels; ++l) { H[l] = levels_host[l].H; W[l] = levels_host[l].W; S[l] = levels_host[l].stride; }
    LocGrid g;
    if (int rc = make_grid(H, W, S, n_levels, B, g)) return rc;
    if (B == 0) return BXI_OK;
    FlatGrid f;
    const int chan[1] = {C};
    const int64_t focal_blocks = make_flat(g, chan, 1, f);
    if (focal_blocks < 0) return BXI_ERR_BAD_SHAPE;
    if (!(gamma >= 0.f) || alpha != alpha || !(eps > 0.f) || loss_weight_cls != loss_weight_cls || loss_weight_bbox != loss_weight_bbox ||
        loss_weight_ctr != loss_weight_ctr)
        return BXI_ERR_BAD_ARGUMENT;
    if (bbox_loss_kind < BXI_FCOS_BBOX_GIOU || bbox_loss_kind > BXI_FCOS_BBOX_IOU_SQUARE) return BXI_ERR_UNSUPPORTED;
    if (!grads_host || !labels || !bbox_targets || !ctr_targets || !norm || !losses) return BXI_ERR_NULL_POINTER;
    Maps m;
    for (int l = 0; l < kMaxL; ++l) {
        if (l < n_levels) {
            const bxi_det_level& a = levels_host[l];
            const bxi_fcos_grads& o = grads_host[l];
            if (!a.cls || !a.bbox || !a.ctr || !o.cls || !o.bbox || !o.ctr) return BXI_ERR_NULL_POINTER;
            m.cls[l] = a.cls; m.bbox[l] = a.bbox; m.ctr[l] = a.ctr;
            m.gcls[l] = o.cls; m.gbbox[l] = o.bbox; m.gctr[l] = o.ctr;
        } else {
            m.cls[l] = m.bbox[l] = m.ctr[l] = nullptr;
            m.gcls[l] = m.gbbox[l] = m.gctr[l] = nullptr;
        }
    }
    const int loc_blocks = g.blk_first[g.n];
    const int n_blocks = (int)focal_blocks + loc_blocks;
    if (!workspace_ok(workspace, workspace_bytes, 16 * (size_t)n_blocks, 4)) return BXI_ERR_WORKSPACE;
    hipStream_t s = as_stream(stream);
    int32_t* part = static_cast<int32_t*>(workspace);
    if (gamma == 2.f)
        BXI_LAUNCH("fcos_focal_g2", s, fcos_focal_kernel<true>, dim3((unsigned)focal_blocks), dim3(256), 0, s, m, g, f, C, labels, norm, gamma,
                   alpha, loss_weight_cls, part, 0);
    else
        BXI_LAUNCH("fcos_focal", s, fcos_focal_kernel<false>, dim3((unsigned)focal_blocks), dim3(256), 0, s, m, g, f, C, labels, norm, gamma, alpha,
                   loss_weight_cls, part, 0);
    if (int rc = check_launch()) return rc;
    BXI_LAUNCH("fcos_pos", s, fcos_pos_kernel, dim3((unsigned)loc_blocks), dim3(kLocTile), 0, s, m, g, C, labels, bbox_targets, ctr_targets, norm,
               loss_weight_bbox, loss_weight_ctr, bbox_loss_kind, eps, part, (int)focal_blocks);
    if (int rc = check_launch()) return rc;
    BXI_LAUNCH("fcos_loss_finish", s, fcos_finish_kernel, dim3(1), dim3(256), 0, s, part, n_blocks, 1, losses, (int32_t*)nullptr);
    return check_launch();
}

extern "C" int bxi_fcos_grad_rescale_f32(const bxi_fcos_level* levels_host, int n_levels, int B, int C, const bxi_fcos_grads* unit_host,
                                         const float* upstream, const bxi_fcos_grads* out_host, void* stream) {
    LocGrid g;
    if (int rc = grid_of(levels_host, n_levels, B, g)) return rc;
    if (C < 1) return BXI_ERR_BAD_SHAPE;
    if (B == 0) return BXI_OK;
    FlatGrid f;
    const int chan[3] = {C, 4, 1};
    const int64_t blocks = make_flat(g, chan, 3, f);
    if (blocks < 0) return BXI_ERR_BAD_SHAPE;
    if (!unit_host || !out_host || !upstream) return BXI_ERR_NULL_POINTER;
    RescaleSegs sg;
    for (int s = 0; s < 3 * kMaxL; ++s) {
        sg.src[s] = nullptr; sg.dst[s] = nullptr; sg.which[s] = 0;
        if (s < f.n) {
            const int l = s / 3, k = s - 3 * l;
            sg.src[s] = k == 0 ? unit_host[l].cls : (k == 1 ? unit_host[l].bbox : unit_host[l].ctr);
            sg.dst[s] = k == 0 ? out_host[l].cls : (k == 1 ? out_host[l].bbox : out_host[l].ctr);
            sg.which[s] = k;
            if (!sg.src[s] || !sg.dst[s]) return BXI_ERR_NULL_POINTER;
        }
    }
    hipStream_t s = as_stream(stream);
    BXI_LAUNCH("fcos_grad_rescale", s, flat_rescale_kernel, dim3((unsigned)blocks), dim3(256), 0, s, sg, f, upstream);
    return check_launch();
}
