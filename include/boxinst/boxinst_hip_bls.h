/*
 * boxinst_hip_bls.h -- the mask losses of BoxSOLOv2Head.loss (BoxLevelSet) for the set cells of ALL levels in libboxinst_hip.so: the
 * scores, the projection term, pixel_num and the image level-set energy in one pass over the logits, the level-set energy on the rows'
 * own tree-filter outputs, and one backward launch that writes every element of every level's gradient.  gfx950 (MI355X / CDNA4) only.
 *
 * An additive part of the C ABI: the conventions, the status codes and BXI_ABI_VERSION are those of ../boxinst_hip.h (device pointers
 * owned by the caller, state-free, allocation-free, asynchronous on `stream`, hipGraph capturable, BXI_OK or a negative bxi_status).
 * No entry point synchronises, reads a device value on the host, calls memset or uses a float atomic; every sum has a fixed order, so
 * two runs are bit-identical; every element of every output and of `state` is written exactly once per call.  Paths are relative to the
 * upstream checkout of the reference (LiWentomng/BoxInstSeg):
 *   head.py  = mmdet/models/dense_heads/box_solov2_head.py   (:293-367, the mask part of loss)
 *   proj.py  = mmdet/models/losses/box_projection_loss.py    (:18-42)
 *   ls.py    = mmdet/models/losses/levelset_loss.py          (:29-44 region_levelset)
 *
 * ROWS AND SIZE GROUPS.  A row is one set cell (level, image, cell).  Levels of one output size form a size group; group g has its own
 * (h, w), its image [B,3,h,w] (the normalised image resized to the group's size) and its target planes masks [G,h,w] uint8 (the compact
 * masks of the targets, read as bytes: zero / not zero).  The rows are numbered group by group -- group 0's rows first --; inside a group
 * the caller chooses the order (the Python layer uses (image, level, cell), so that an image's rows of a group are contiguous and form
 * the channels of one tree-filter call).  Row m of group g owns
 *   - h w consecutive floats of every ragged per-pixel buffer (p, g_p, y_img, y_lst ...) at sum_{g' < g} rows_g' h_g' w_g' + r h w,
 *     r = m - (first row of g);
 *   - row_src[m] = level * BXI_BLS_LEVEL_ROWS + n: its logit plane is plane n of level tensor `level` [N_level, h, w].  The level
 *     tensors are separate allocations, passed as a HOST array of device pointers and read in place: nothing is stacked or copied.
 *     The backward writes the row's gradient to the same plane of the level's gradient tensor, so the rows of a call must name every
 *     plane of every level exactly once (a bijection: the set cells ARE the planes of box_solov2_ins_preds);
 *   - tgt_of[m]: its ground truth among the group's G;   img_of[m]: its image among B.
 * INERT ROWS.  tgt_of or img_of of -1 -- or any index outside its range: nothing is read through it -- makes the row inert: its scores
 * are zeros, its losses 0, live[m] = 0, pixel_num[m] = 1 and its plane of the level's gradient is zeros.  A row whose row_src is out
 * of range is inert as well and has no plane to write.
 *
 * WORK.  A workgroup serves a chunk of BXI_BLS_CHUNK_PIXELS / w (at least 1) lines of one row, so a row of a small group costs what
 * its pixels cost.  Common support set: fp32, 1 <= groups <= BXI_BLS_MAX_GROUPS, 1 <= levels <= BXI_BLS_MAX_LEVELS, h, w >= 1,
 * w <= BXI_BLS_MAX_W, M = sum rows <= 65535 and < BXI_BLS_LEVEL_ROWS per level, every ragged buffer within int32.  More groups, levels
 * or columns: BXI_ERR_UNSUPPORTED; a non-positive size, negative count, a level of another size than its group or row counts that do
 * not add up: BXI_ERR_BAD_SHAPE; a NULL pointer that a launch would read or write: BXI_ERR_NULL_POINTER; state NULL, too small or not
 * 8-byte aligned: BXI_ERR_WORKSPACE.  M == 0 is a no-op.  Nothing is launched on an error.
 */
#ifndef BOXINST_HIP_BLS_H
#define BOXINST_HIP_BLS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BXI_BLS_MAX_GROUPS 4          /* size groups per call (the rescale factors of boxinst_hip_solo.h) */
#define BXI_BLS_MAX_LEVELS 8          /* level tensors per call */
#define BXI_BLS_MAX_W 2048            /* columns of a plane: the column maxima of a chunk live in the LDS */
#define BXI_BLS_CHUNK_PIXELS 1024     /* a workgroup's chunk: max(1, BXI_BLS_CHUNK_PIXELS / w) lines of one row */
#define BXI_BLS_LEVEL_ROWS (1 << 20)  /* row_src = level * BXI_BLS_LEVEL_ROWS + plane */

struct bxi_bls_group {
    const float* img;       /* [B,3,h,w] */
    const uint8_t* masks;   /* [G,h,w] */
    int h, w, rows, G;      /* rows: the rows of this group, consecutive in every per-row array */
};

/* Bytes of `state` (8-byte aligned; 0 for a table the entry points refuse): per row the saved sums of both level-set terms and of the
 * dice terms, per line and per column the arg-max with the target's projection bit, and the chunks' partial sums. */
size_t bxi_bls_state_bytes(const struct bxi_bls_group* groups_host, int n_groups);

/* bxi_bls_front_f32  <->  head.py:338-351 and proj.py for the rows of all groups, in TWO launches (chunk partials, then one workgroup
 * per row).  One pass over each row's logits x gives
 *   p = sigmoid(x), written to the ragged buffer;
 *   loss_proj [M] = w_proj (dice(max over a column, target's column projection) + dice(max over a line, target's line projection)):
 *     the maxima are taken with the project's arg-max rule, the first index of the largest LOGIT (the backward sends the gradient there);
 *     the target's projections are an OR of the bytes; dice = 1 - 2 sum(x t) / (sum x^2 + sum t^2 + 1e-5), sums in fp64;
 *   pixel_num [M] = max(number of target bytes that are not zero, 1), an exact integer count (head.py:348-349);
 *   loss_img [M] = w_img energy / (3 pixel_num), energy = region_levelset((p T, (1 - p) T), img T) of ls.py:29-44 with f = p T,
 *     g = (1 - p) T and t = img T formed in registers and rounded to fp32 as the reference's stored tensors are, in the one-pass form
 *     (sum g t^2 - 2 a sum g t + a^2 sum g) with fp64 partials per chunk combined in index order and the 1e-5 clamps of ls.py:37-38;
 *     w_img carries head.py:351's 0.05;
 *   live [M] = 1.0 for a row that is not inert, else 0.0.
 * levels_host [L]: HOST array of device pointers (NULL allowed for a level without planes); level_rows_host [L]: planes per level;
 * level_group_host [L]: the group of each level. */
int bxi_bls_front_f32(const struct bxi_bls_group* groups_host, int n_groups, const float* const* levels_host, const int* level_rows_host,
                      const int* level_group_host, int L, const int32_t* row_src, const int32_t* tgt_of, const int32_t* img_of, int M, int B,
                      double w_proj, double w_img, float* p, float* loss_proj, float* loss_img, float* pixel_num, float* live, void* state,
                      size_t state_bytes, void* stream);

/* bxi_bls_backward_f32: ONE launch writes every element of every level's gradient tensor (grads_host [L]: HOST array of device
 * pointers, [N_level,h,w] each).  Per element (g_proj + g_img_levelset + g_p) p (1 - p):
 *   g_proj          at the line's and at the column's arg-max position: g_loss_proj[m] w_proj d dice / d x;
 *   g_img_levelset  g_loss_img[m] times the derivative of loss_img through f and g, from the saved region means;
 *   g_p             the incoming gradient of the scores [ragged]: the filter path's plus bxi_bls_high_backward_f32's direct one.
 * Inert rows get zeros.  p, state: what bxi_bls_front_f32 wrote for the same table. */
int bxi_bls_backward_f32(const struct bxi_bls_group* groups_host, int n_groups, float* const* grads_host, const int* level_rows_host,
                         const int* level_group_host, int L, const int32_t* row_src, const int32_t* tgt_of, const int32_t* img_of, int M, int B,
                         double w_proj, double w_img, const float* p, const float* g_p, const float* g_loss_proj, const float* g_loss_img,
                         const void* state, size_t state_bytes, void* stream);

/* Bytes of `state` of the pair below (8-byte aligned; 0 for a table the entry points refuse). */
size_t bxi_bls_high_state_bytes(const struct bxi_bls_group* groups_host, int n_groups);

/* bxi_bls_high_forward_f32  <->  head.py:358-360: loss_levelset(mask_scores_phi, cat(y_img, y_lst) T, pixel_num) -- the ragged sibling
 * of bxi_b2m_levelset_forward_f32 with shared == 0 and C = 2: the target's two channels are the rows' own filter outputs y_img, y_lst
 * [ragged, as p], multiplied by T in registers.  loss [M] = weight energy / (2 pixel_num[m]); weight carries head.py:360's 5.0.
 * live, pixel_num [M]: what bxi_bls_front_f32 wrote; a row with live == 0 is inert here too.  groups[g].img is not read.  Two launches. */
int bxi_bls_high_forward_f32(const struct bxi_bls_group* groups_host, int n_groups, const float* p, const float* y_img, const float* y_lst,
                             const int32_t* tgt_of, const float* live, const float* pixel_num, int M, double weight, float* loss, void* state,
                             size_t state_bytes, void* stream);

/* Its backward, one launch: g_p [ragged] (both score channels folded: T (g_fore - g_back)) and g_y_img, g_y_lst [ragged], already
 * multiplied by T.  Every element of the three is written; inert rows get zeros. */
int bxi_bls_high_backward_f32(const struct bxi_bls_group* groups_host, int n_groups, const float* p, const float* y_img, const float* y_lst,
                              const int32_t* tgt_of, const float* live, const float* pixel_num, int M, double weight, const void* state,
                              size_t state_bytes, const float* g_loss, float* g_p, float* g_y_img, float* g_y_lst, void* stream);

#ifdef __cplusplus
}
#endif
#endif
