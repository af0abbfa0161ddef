// The entry points that take no net: image input (resize, letterbox and its inverse), evaluation counters, validation loss, the
// TFRecord checksum, decode and class scores, NMS and the packing of detections.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "y3_host.h"

namespace y3 {
// include/y3.h, Y3_IMAGE_LETTERBOX.  Every operation in fp32 (this file is compiled with -ffp-contract=off), nearbyintf in the
// default rounding mode (half to even): bit for bit what core/utils.letterbox_geometry computes with np.float32 and np.rint.
LetterboxGeom letterbox_geom(int h, int w, int Hc, int Wc)
{
    const float scale = std::min((float)Hc / (float)h, (float)Wc / (float)w);
    LetterboxGeom g;
    g.sh = std::max(1, (int)nearbyintf(scale * (float)h));
    g.sw = std::max(1, (int)nearbyintf(scale * (float)w));
    g.top = (Hc - g.sh) >> 1;      // floor, also where the difference is negative (refused by letterbox_geom_fits)
    g.left = (Wc - g.sw) >> 1;
    return g;
}
}  // namespace y3

// ------------------------------------------------------------------------------------------ image input
namespace {
// is_uint8 / y3_image_desc.mode: 0, 1 or 2, with or without Y3_IMAGE_LETTERBOX
bool image_mode_ok(int mode) { return (mode & ~Y3_IMAGE_LETTERBOX) >= 0 && (mode & ~Y3_IMAGE_LETTERBOX) <= 2; }
// the geometry of one image: the whole canvas without the flag
y3::LetterboxGeom image_geom(int mode, int h, int w, int Hc, int Wc)
{
    return (mode & Y3_IMAGE_LETTERBOX) ? y3::letterbox_geom(h, w, Hc, Wc) : y3::LetterboxGeom{Hc, Wc, 0, 0};
}
// the window ch x cw at (y0, x0) lies inside h x w
bool window_in_frame(int y0, int x0, int ch, int cw, int h, int w)
{
    return ch >= 1 && cw >= 1 && y0 >= 0 && x0 >= 0 && y0 <= h - ch && x0 <= w - cw;
}

// A descriptor in window form is a y3_tile_desc, and an image is the whole-frame window of itself.
y3_tile_desc as_window(const y3_image_desc &d) { return {d.offset, d.height, d.width, d.channels, d.mode, 0, 0, d.height, d.width}; }
const y3_tile_desc &as_window(const y3_tile_desc &d) { return d; }

struct Blob { const void *dev; size_t bytes; };

// The one check of a descriptor, and the view preprocess_batch_kernel reads for it: `noun` i ("image" / "tile") in the messages.
// blob null: what the geometry calls check -- mode, extent and window; channels and offset are not read and `view` gets the geometry only.
y3_status resize_view(const char *who, const char *noun, int i, const y3_tile_desc &d, const Blob *blob, int Hc, int Wc, y3::ResizeView *view)
{
    if (blob && (d.channels < 3 || d.channels > 4))
        return fail(Y3_ERR_INVALID, "%s: %s %d: channels must be 3 or 4 (got %d)", who, noun, i, d.channels);
    if (!image_mode_ok(d.mode))
        return fail(Y3_ERR_INVALID, "%s: %s %d: mode must be 0, 1 or 2, optionally | Y3_IMAGE_LETTERBOX (got %d)", who, noun, i, d.mode);
    if (d.height < 1 || d.width < 1)
        return fail(Y3_ERR_INVALID, "%s: %s %d: height and width must be at least 1 (got %d x %d)", who, noun, i, d.height, d.width);
    if (d.ch < 1 || d.cw < 1) return fail(Y3_ERR_INVALID, "%s: %s %d: ch and cw must be at least 1 (got %d x %d)", who, noun, i, d.ch, d.cw);
    if (!window_in_frame(d.y0, d.x0, d.ch, d.cw, d.height, d.width))
        return fail(Y3_ERR_INVALID, "%s: %s %d: window %d x %d at (%d, %d) does not lie inside the %d x %d image", who, noun, i, d.ch, d.cw,
                    d.y0, d.x0, d.height, d.width);
    view->g = image_geom(d.mode, d.ch, d.cw, Hc, Wc);
    if (!blob) return Y3_OK;
    const bool f32 = (d.mode & ~Y3_IMAGE_LETTERBOX) == 0;
    if (f32 && ((d.offset & 3) || ((uintptr_t)blob->dev & 3)))
        return fail(Y3_ERR_INVALID, "%s: %s %d: float32 pixels must be 4-byte aligned (offset %llu)", who, noun, i,
                    (unsigned long long)d.offset);
    // height, width < 2^31 and channels * elemsize <= 16: the product stays below 2^66, so take it in 128 bits
    const unsigned pixel_bytes = (unsigned)(d.channels * (f32 ? 4 : 1));
    const unsigned __int128 bytes = (unsigned __int128)d.height * (unsigned __int128)d.width * pixel_bytes;
    if ((unsigned __int128)d.offset + bytes > (unsigned __int128)blob->bytes)
        return fail(Y3_ERR_INVALID, "%s: %s %d: %d x %d x %d at offset %llu runs past the %zu-byte pixel blob", who, noun, i,
                    d.height, d.width, d.channels, (unsigned long long)d.offset, blob->bytes);
    if (!y3::letterbox_geom_fits(view->g, Hc, Wc))
        return fail(Y3_ERR_INVALID, "%s: %s %d: letterbox of %d x %d (%d x %d at %d, %d) does not fit %d x %d", who, noun, i,
                    d.ch, d.cw, view->g.sh, view->g.sw, view->g.top, view->g.left, Hc, Wc);
    view->first = d.offset + ((uint64_t)d.y0 * d.width + d.x0) * pixel_bytes;     // inside the blob: 64 bits hold it
    view->rows = d.ch, view->cols = d.cw, view->pitch_px = d.width, view->channels = d.channels, view->mode = d.mode;
    return Y3_OK;
}

// y3_preprocess_batch[_hw] (Desc = y3_image_desc) and y3_preprocess_tiles_hw (y3_tile_desc)
template <typename Desc>
y3_status preprocess_views(const char *who, const char *noun, const void *pixels_dev, size_t pixels_bytes, const Desc *descs_host, int n,
                           float *batch_dev, int first_slot, int Hc, int Wc, void *stream)
{
    if (!pixels_dev || !descs_host || !batch_dev || n < 1 || first_slot < 0 || Hc <= 0 || Wc <= 0)
        return fail(Y3_ERR_INVALID, "%s: bad argument (null pointer, n_%ss < 1, first_slot < 0 or canvas <= 0)", who, noun);
    const Blob blob{pixels_dev, pixels_bytes};
    y3::ResizeTable table{};     // on the stack: the call allocates nothing
    // every check before the first launch: a bad descriptor late in the list must not leave the batch half written
    for (int i = 0; i < n; ++i)
        if (y3_status st = resize_view(who, noun, i, as_window(descs_host[i]), &blob, Hc, Wc, &table.v[0]); st != Y3_OK) return st;
    const size_t per_image = (size_t)Hc * Wc * 3;
    for (int i0 = 0; i0 < n; i0 += y3::kResizeTableViews) {
        const int m = std::min(y3::kResizeTableViews, n - i0);
        for (int i = 0; i < m; ++i) resize_view(who, noun, i0 + i, as_window(descs_host[i0 + i]), &blob, Hc, Wc, &table.v[i]);
        hipError_t e = y3::launch_preprocess_batch(pixels_dev, table, m, batch_dev + ((size_t)first_slot + i0) * per_image, Hc, Wc,
                                                   (hipStream_t)stream);
        if (e != hipSuccess) return fail(Y3_ERR_HIP, "%s launch: %s", who, hipGetErrorString(e));
    }
    return Y3_OK;
}

// y3_letterbox_geometry[_hw] and y3_tile_letterbox_geometry_hw: nothing is written unless every descriptor passes
template <typename Desc>
y3_status view_geometries(const char *who, const char *noun, const Desc *descs_host, int n, int Hc, int Wc, int32_t *geoms_out_host)
{
    if (!descs_host || !geoms_out_host || n < 1 || Hc <= 0 || Wc <= 0)
        return fail(Y3_ERR_INVALID, "%s: bad argument (null pointer, n_%ss < 1 or canvas <= 0)", who, noun);
    static_assert(sizeof(y3::LetterboxGeom) == 4 * sizeof(int32_t), "a geometry is four int32");
    y3::ResizeView v;
    for (int i = 0; i < n; ++i)
        if (y3_status st = resize_view(who, noun, i, as_window(descs_host[i]), nullptr, Hc, Wc, &v); st != Y3_OK) return st;
    for (int i = 0; i < n; ++i) {
        resize_view(who, noun, i, as_window(descs_host[i]), nullptr, Hc, Wc, &v);
        memcpy(geoms_out_host + (size_t)i * 4, &v.g, sizeof(v.g));
    }
    return Y3_OK;
}
}  // namespace

// ------------------------------------------------------------------------------------------ decode
// gs: grid_hw[ns][2] = {gh, gw} per scale (the square entry points hand {g, g}); ns: scales, 1..3 (the three-scale entry points hand 3)
// The checks every decode entry shares, and the by-value arguments of its launch: grid sizes, first box of each scale, anchors
static y3_status decode_args(const float *const *grids, const int32_t (*gs)[2], int ns, int batch, int nc, const float *anchors, const char *who,
                             y3::DecodeArgs *out)
{
    if (!grids || !gs || !anchors || batch <= 0 || nc <= 0) return fail(Y3_ERR_INVALID, "%s: bad argument", who);
    if (ns < 1 || ns > 3) return fail(Y3_ERR_INVALID, "%s: 1 to 3 scales (got %d)", who, ns);
    y3::DecodeArgs a{};   // a scale behind ns stays empty: no boxes, no workgroup
    int off = 0;
    for (int s = 0; s < ns; ++s) {
        if (!grids[s] || gs[s][0] <= 0 || gs[s][1] <= 0 || ((uintptr_t)grids[s] & 15))
            return fail(Y3_ERR_INVALID, "%s: grid %d null, empty or not 16-byte aligned", who, s);
        a.grid[s] = grids[s];
        a.gh[s] = gs[s][0];
        a.gw[s] = gs[s][1];
        a.off[s] = off;
        off += gs[s][0] * gs[s][1] * 3;
        for (int k = 0; k < 3; ++k) {
            a.anchors[s][k][0] = anchors[(s * 3 + k) * 2 + 0];
            a.anchors[s][k][1] = anchors[(s * 3 + k) * 2 + 1];
        }
    }
    a.B = batch;
    a.N = off;
    a.nc = nc;
    *out = a;
    return Y3_OK;
}

static y3_status decode_common(const float *const *grids, const int32_t (*gs)[2], int ns, int batch, int nc,
                               const float *anchors, float *bboxes, float *conf, float *probs, int64_t *cls,
                               float *scores, void *stream, const char *who)
{
    if (!bboxes) return fail(Y3_ERR_INVALID, "%s: bad argument", who);
    y3::DecodeArgs a{};
    if (y3_status st = decode_args(grids, gs, ns, batch, nc, anchors, who, &a); st != Y3_OK) return st;
    if ((uintptr_t)bboxes & 15) return fail(Y3_ERR_INVALID, "%s: bboxes not 16-byte aligned", who);
    hipError_t e = y3::launch_decode(a, bboxes, conf, probs, cls, scores, (hipStream_t)stream);
    if (e != hipSuccess) return fail(Y3_ERR_HIP, "%s launch: %s", who, hipGetErrorString(e));
    return Y3_OK;
}

// boxes per image of the ns grids, 0 when ns is not 1..3, a side is < 1 or the count leaves an int
static long long grid_boxes(const int32_t (*gs)[2], int ns)
{
    long long n = 0;
    if (ns < 1 || ns > 3) return 0;
    for (int s = 0; s < ns; ++s) {
        if (gs[s][0] <= 0 || gs[s][1] <= 0) return 0;
        n += 3ll * gs[s][0] * gs[s][1];
    }
    return n <= 0x7fffffffll ? n : 0;
}

y3_status y3::decode_candidates_hw(const char *who, const float *const *grids_dev, const int32_t (*grid_hw)[2], int n_scales, int batch, int nclasses,
                                   const float *anchors_host, float score_threshold, int capacity, float *cand_boxes_dev,
                                   int64_t *cand_cls_dev, float *cand_scores_dev, int32_t *cand_src_dev, int32_t *totals_dev,
                                   void *workspace_dev, size_t workspace_bytes, void *stream)
{
    if (!grids_dev || !grid_hw || !anchors_host || !cand_boxes_dev || !cand_cls_dev || !cand_scores_dev || !cand_src_dev || !totals_dev)
        return fail(Y3_ERR_INVALID, "%s: null pointer", who);
    if (batch < 1 || capacity < 1 || nclasses < 1)
        return fail(Y3_ERR_INVALID, "%s: batch, capacity and nclasses must be at least 1 (got %d, %d, %d)", who, batch, capacity, nclasses);
    if (n_scales < 1 || n_scales > 3) return fail(Y3_ERR_INVALID, "%s: 1 to 3 scales (got %d)", who, n_scales);
    const long long N = grid_boxes(grid_hw, n_scales);
    if (N <= 0) return fail(Y3_ERR_INVALID, "%s: grid sides must be at least 1 and the boxes per image below 2^31", who);
    if ((long long)batch * capacity > 0x7fffffffll || N * nclasses > 0x7fffffffll || (long long)batch * N > 0x7fffffffll)
        return fail(Y3_ERR_INVALID, "%s: batch * capacity, N * nclasses and batch * N must stay below 2^31 (got %d x %d, %lld x %d)", who, batch,
                    capacity, N, nclasses);
    if (y3::decode_lds_bytes(nclasses) > 160 * 1024)
        return fail(Y3_ERR_INVALID, "%s: %d classes need %zu bytes of LDS, at most %d", who, nclasses, y3::decode_lds_bytes(nclasses), 160 * 1024);
    y3::DecodeArgs a{};
    if (y3_status st = decode_args(grids_dev, grid_hw, n_scales, batch, nclasses, anchors_host, who, &a); st != Y3_OK) return st;
    if ((uintptr_t)cand_boxes_dev & 15) return fail(Y3_ERR_INVALID, "%s: cand_boxes not 16-byte aligned", who);
    if (((uintptr_t)cand_cls_dev & 7) || ((uintptr_t)cand_scores_dev & 3) || ((uintptr_t)cand_src_dev & 3) || ((uintptr_t)totals_dev & 3))
        return fail(Y3_ERR_INVALID, "%s: cand_cls not 8-byte or cand_scores / cand_src / totals not 4-byte aligned", who);
    const size_t need = (size_t)batch * (size_t)N * sizeof(int32_t);
    if (!workspace_dev || workspace_bytes < need || ((uintptr_t)workspace_dev & 3))
        return fail(Y3_ERR_INVALID, "%s: workspace too small or not 4-byte aligned (need %zu bytes)", who, need);
    hipError_t e = y3::launch_candidates(a, score_threshold, capacity, cand_boxes_dev, cand_cls_dev, cand_scores_dev, cand_src_dev, totals_dev,
                                         static_cast<int32_t *>(workspace_dev), (hipStream_t)stream);
    if (e != hipSuccess) return fail(Y3_ERR_HIP, "%s launch: %s", who, hipGetErrorString(e));
    return Y3_OK;
}

// The square entry points are the _hw ones with {g, g}; `who` names the entry point the caller used in the messages.
static y3_status yolo_decode_hw(const char *who, const float *const *grids_dev, const int32_t (*grid_hw)[2], int n_scales, int batch, int nclasses,
                                const float *anchors_host, float *bboxes_dev, float *conf_dev, float *probs_dev, void *stream)
{
    if (!conf_dev || !probs_dev) return fail(Y3_ERR_INVALID, "%s: null output", who);
    return decode_common(grids_dev, grid_hw, n_scales, batch, nclasses, anchors_host, bboxes_dev, conf_dev, probs_dev, nullptr, nullptr, stream, who);
}

y3_status y3::decode_scores_hw(const char *who, const float *const *grids_dev, const int32_t (*grid_hw)[2], int n_scales, int batch, int nclasses,
                               const float *anchors_host, float *bboxes_dev, int64_t *class_idx_dev, float *scores_dev, void *stream)
{
    if (!class_idx_dev || !scores_dev) return fail(Y3_ERR_INVALID, "%s: null output", who);
    return decode_common(grids_dev, grid_hw, n_scales, batch, nclasses, anchors_host, bboxes_dev, nullptr, nullptr, class_idx_dev, scores_dev, stream, who);
}

extern "C" {

// The square entry points (y3_preprocess_image, ...) are their _hw counterparts with canvas_h == canvas_w; `who` names the
// entry point the caller used in the messages.
static y3_status preprocess_image_hw(const char *who, const void *image_dev, int is_uint8, int height, int width, int channels,
                                     float *batch_dev, int slot, int Hc, int Wc, void *stream)
{
    if (!image_dev || !batch_dev || height <= 0 || width <= 0 || channels < 3 || channels > 4 || slot < 0 ||
        Hc <= 0 || Wc <= 0 || !image_mode_ok(is_uint8) || ((is_uint8 & ~Y3_IMAGE_LETTERBOX) == 0 && ((uintptr_t)image_dev & 3)))
        return fail(Y3_ERR_INVALID, "%s: bad argument (channels must be 3 or 4)", who);
    const y3::LetterboxGeom g = image_geom(is_uint8, height, width, Hc, Wc);
    if (!y3::letterbox_geom_fits(g, Hc, Wc))
        return fail(Y3_ERR_INVALID, "%s: letterbox of %d x %d (%d x %d at %d, %d) does not fit %d x %d", who, height, width,
                    g.sh, g.sw, g.top, g.left, Hc, Wc);
    float *dst = batch_dev + (size_t)slot * Hc * Wc * 3;
    hipError_t e = y3::launch_resize(image_dev, is_uint8, height, width, channels, dst, Hc, Wc, g, (hipStream_t)stream);
    if (e != hipSuccess) return fail(Y3_ERR_HIP, "%s launch: %s", who, hipGetErrorString(e));
    return Y3_OK;
}

y3_status y3_preprocess_image_hw(const void *image_dev, int is_uint8, int height, int width, int channels,
                                 float *batch_dev, int slot, int canvas_h, int canvas_w, void *stream)
try {
    return preprocess_image_hw("y3_preprocess_image_hw", image_dev, is_uint8, height, width, channels, batch_dev, slot, canvas_h, canvas_w, stream);
}
Y3_CATCH("y3_preprocess_image_hw")

y3_status y3_preprocess_image(const void *image_dev, int is_uint8, int height, int width, int channels,
                              float *batch_dev, int slot, int image_size, void *stream)
try {
    return preprocess_image_hw("y3_preprocess_image", image_dev, is_uint8, height, width, channels, batch_dev, slot, image_size, image_size, stream);
}
Y3_CATCH("y3_preprocess_image")

y3_status y3_preprocess_batch_hw(const void *pixels_dev, size_t pixels_bytes, const y3_image_desc *descs_host, int n_images,
                                 float *batch_dev, int first_slot, int canvas_h, int canvas_w, void *stream)
try {
    return preprocess_views("y3_preprocess_batch_hw", "image", pixels_dev, pixels_bytes, descs_host, n_images, batch_dev, first_slot, canvas_h, canvas_w, stream);
}
Y3_CATCH("y3_preprocess_batch_hw")

y3_status y3_preprocess_batch(const void *pixels_dev, size_t pixels_bytes, const y3_image_desc *descs_host, int n_images,
                              float *batch_dev, int first_slot, int image_size, void *stream)
try {
    return preprocess_views("y3_preprocess_batch", "image", pixels_dev, pixels_bytes, descs_host, n_images, batch_dev, first_slot, image_size, image_size, stream);
}
Y3_CATCH("y3_preprocess_batch")

y3_status y3_letterbox_geometry_hw(const y3_image_desc *descs_host, int n_images, int canvas_h, int canvas_w, int32_t *geoms_out_host)
try {
    return view_geometries("y3_letterbox_geometry_hw", "image", descs_host, n_images, canvas_h, canvas_w, geoms_out_host);
}
Y3_CATCH("y3_letterbox_geometry_hw")

y3_status y3_letterbox_geometry(const y3_image_desc *descs_host, int n_images, int image_size, int32_t *geoms_out_host)
try {
    return view_geometries("y3_letterbox_geometry", "image", descs_host, n_images, image_size, image_size, geoms_out_host);
}
Y3_CATCH("y3_letterbox_geometry")

static y3_status unletterbox_hw(const char *who, void *packed_dev, const int32_t *num_valid_dev, const int32_t *geoms_host, int batch,
                                int max_boxes, int Hc, int Wc, void *stream)
{
    if (!packed_dev || !num_valid_dev || !geoms_host || batch < 1 || Hc <= 0 || Wc <= 0)
        return fail(Y3_ERR_INVALID, "%s: bad argument (null pointer, batch < 1 or image_size <= 0)", who);
    if (max_boxes <= 0 || max_boxes > Y3_MAX_OUTPUT_BOXES)
        return fail(Y3_ERR_INVALID, "%s: max_boxes must be in [1,%d]", who, Y3_MAX_OUTPUT_BOXES);
    // every check before the first launch: the rows are rewritten in place
    for (int i = 0; i < batch; ++i) {
        y3::LetterboxGeom g;
        memcpy(&g, geoms_host + (size_t)i * 4, sizeof(g));
        if (!y3::letterbox_geom_fits(g, Hc, Wc))
            return fail(Y3_ERR_INVALID, "%s: image %d: geometry %d x %d at (%d, %d) does not lie inside %d x %d", who, i,
                        g.sh, g.sw, g.top, g.left, Hc, Wc);
    }
    unsigned *packed = static_cast<unsigned *>(packed_dev);
    for (int i0 = 0; i0 < batch; i0 += y3::kUnletterboxTableImages) {
        const int n = std::min(y3::kUnletterboxTableImages, batch - i0);
        y3::LetterboxGeom geoms[y3::kUnletterboxTableImages];
        memcpy(geoms, geoms_host + (size_t)i0 * 4, (size_t)n * sizeof(y3::LetterboxGeom));
        hipError_t e = y3::launch_unletterbox(packed + (size_t)i0 * max_boxes * 7, num_valid_dev + i0, geoms, n, max_boxes, Hc, Wc,
                                              (hipStream_t)stream);
        if (e != hipSuccess) return fail(Y3_ERR_HIP, "%s launch: %s", who, hipGetErrorString(e));
    }
    return Y3_OK;
}

y3_status y3_unletterbox_detections_hw(void *packed_dev, const int32_t *num_valid_dev, const int32_t *geoms_host, int batch,
                                       int max_boxes, int canvas_h, int canvas_w, void *stream)
try {
    return unletterbox_hw("y3_unletterbox_detections_hw", packed_dev, num_valid_dev, geoms_host, batch, max_boxes, canvas_h, canvas_w, stream);
}
Y3_CATCH("y3_unletterbox_detections_hw")

y3_status y3_unletterbox_detections(void *packed_dev, const int32_t *num_valid_dev, const int32_t *geoms_host, int batch,
                                    int max_boxes, int image_size, void *stream)
try {
    return unletterbox_hw("y3_unletterbox_detections", packed_dev, num_valid_dev, geoms_host, batch, max_boxes, image_size, image_size, stream);
}
Y3_CATCH("y3_unletterbox_detections")

// ------------------------------------------------------------------------------------------ sliced inference
int y3_tile_grid(int height, int width, int rows, int cols, int overlap_px, int overview, int32_t *out)
{
    const char *who = "y3_tile_grid";
    if (!out) return fail(Y3_ERR_INVALID, "%s: null pointer", who);
    if (height < 1 || width < 1) return fail(Y3_ERR_INVALID, "%s: height and width must be at least 1 (got %d x %d)", who, height, width);
    if (rows < 1 || rows > 8 || cols < 1 || cols > 8) return fail(Y3_ERR_INVALID, "%s: rows and cols must be in [1,8] (got %d x %d)", who, rows, cols);
    if (overlap_px < 0 || overlap_px > std::min(height, width))
        return fail(Y3_ERR_INVALID, "%s: overlap_px must be in [0, min(height, width)] (got %d for %d x %d)", who, overlap_px, height, width);
    const int T = rows * cols + (overview ? 1 : 0);
    if (T > y3::kMergeMaxTiles) return fail(Y3_ERR_INVALID, "%s: %d tiles, at most %d", who, T, y3::kMergeMaxTiles);
    // one axis: the window length, then the origin of window i (64-bit products: e * k stays far below 2^63)
    auto length = [&](int e, int k) { return (int)(((long long)e + (long long)(k - 1) * overlap_px + k - 1) / k); };
    auto origin = [](int e, int len, int k, int i) { return k == 1 ? 0 : (int)((long long)i * (e - len) / (k - 1)); };
    const int lh = length(height, rows), lw = length(width, cols);
    for (int i = 0; i < rows; ++i)
        for (int j = 0; j < cols; ++j) {
            int32_t *o = out + ((size_t)i * cols + j) * 4;
            o[0] = origin(height, lh, rows, i);
            o[1] = origin(width, lw, cols, j);
            o[2] = lh;
            o[3] = lw;
        }
    if (overview) {
        int32_t *o = out + (size_t)rows * cols * 4;
        o[0] = 0, o[1] = 0, o[2] = height, o[3] = width;
    }
    return T;
}

y3_status y3_preprocess_tiles_hw(const void *pixels_dev, size_t pixels_bytes, const y3_tile_desc *descs_host, int n_tiles,
                                 float *batch_dev, int first_slot, int canvas_h, int canvas_w, void *stream)
try {
    return preprocess_views("y3_preprocess_tiles_hw", "tile", pixels_dev, pixels_bytes, descs_host, n_tiles, batch_dev, first_slot, canvas_h, canvas_w, stream);
}
Y3_CATCH("y3_preprocess_tiles_hw")

y3_status y3_tile_letterbox_geometry_hw(const y3_tile_desc *descs_host, int n_tiles, int canvas_h, int canvas_w, int32_t *geoms_out_host)
try {
    return view_geometries("y3_tile_letterbox_geometry_hw", "tile", descs_host, n_tiles, canvas_h, canvas_w, geoms_out_host);
}
Y3_CATCH("y3_tile_letterbox_geometry_hw")

namespace {
// The layout of y3_merge_tile_detections' workspace, every part 16-byte aligned: candidate boxes [F,N,4] f32, class ids [F,N] i64, scores
// [F,N] f32, selected indices [F,M] i32, then the NMS workspace of (F, N) -- the per-class one, which serves either rule.  N = tiles * max_boxes.
struct MergeLayout { size_t boxes, cls, scores, sel, nms, nms_bytes, total; };
bool merge_sizes_ok(int frames, int tiles, int max_boxes)
{
    return frames >= 1 && tiles >= 1 && tiles <= y3::kMergeMaxTiles && max_boxes >= 1 && max_boxes <= Y3_MAX_OUTPUT_BOXES &&
           (unsigned long long)frames * tiles * max_boxes <= 0x7fffffffull;
}
MergeLayout merge_layout(int frames, int tiles, int max_boxes)
{
    const size_t F = frames, N = (size_t)tiles * max_boxes, M = max_boxes;
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    MergeLayout l{};
    l.boxes = 0;
    l.cls = up(l.boxes + F * N * 4 * sizeof(float));
    l.scores = up(l.cls + F * N * sizeof(int64_t));
    l.sel = up(l.scores + F * N * sizeof(float));
    l.nms = up(l.sel + F * M * sizeof(int32_t));
    l.nms_bytes = y3::nms_per_class_workspace_bytes(frames, (int)N);
    l.total = l.nms + l.nms_bytes;
    return l;
}
}  // namespace

size_t y3_merge_tiles_workspace_bytes(int frames, int tiles, int max_boxes)
{
    return merge_sizes_ok(frames, tiles, max_boxes) ? merge_layout(frames, tiles, max_boxes).total : 0;
}

y3_status y3_merge_tile_detections(const void *packed_dev, const int32_t *num_valid_dev, const int32_t *tiles_host,
                                   const int32_t *geoms_host, const int32_t *frame_hw_host, int frames, int tiles, int max_boxes,
                                   int canvas_h, int canvas_w, int nms_mode, float iou_threshold, float score_threshold,
                                   void *packed_out_dev, int32_t *num_valid_out_dev, void *workspace_dev, size_t workspace_bytes,
                                   void *stream)
try {
    const char *who = "y3_merge_tile_detections";
    const int Hc = canvas_h, Wc = canvas_w;
    if (!packed_dev || !num_valid_dev || !tiles_host || !geoms_host || !frame_hw_host || !packed_out_dev || !num_valid_out_dev)
        return fail(Y3_ERR_INVALID, "%s: null pointer", who);
    if (frames < 1) return fail(Y3_ERR_INVALID, "%s: frames must be at least 1 (got %d)", who, frames);
    if (tiles < 1 || tiles > y3::kMergeMaxTiles) return fail(Y3_ERR_INVALID, "%s: tiles must be in [1,%d] (got %d)", who, y3::kMergeMaxTiles, tiles);
    if (max_boxes < 1 || max_boxes > Y3_MAX_OUTPUT_BOXES)
        return fail(Y3_ERR_INVALID, "%s: max_boxes must be in [1,%d] (got %d)", who, Y3_MAX_OUTPUT_BOXES, max_boxes);
    if (!merge_sizes_ok(frames, tiles, max_boxes))
        return fail(Y3_ERR_INVALID, "%s: frames * tiles * max_boxes must stay below 2^31 (got %d x %d x %d)", who, frames, tiles, max_boxes);
    if (Hc <= 0 || Wc <= 0) return fail(Y3_ERR_INVALID, "%s: canvas must be at least 1 x 1 (got %d x %d)", who, Hc, Wc);
    if (nms_mode != Y3_NMS_AGNOSTIC && nms_mode != Y3_NMS_PER_CLASS)
        return fail(Y3_ERR_INVALID, "%s: nms_mode must be Y3_NMS_AGNOSTIC or Y3_NMS_PER_CLASS (got %d)", who, nms_mode);
    if (y3_status st = y3::select_check(who, nms_mode, iou_threshold, score_threshold); st != Y3_OK) return st;   // nothing may be enqueued by a refused call
    for (int f = 0; f < frames; ++f) {
        const int h = frame_hw_host[f * 2], w = frame_hw_host[f * 2 + 1];
        if (h < 1 || w < 1) return fail(Y3_ERR_INVALID, "%s: frame %d: height and width must be at least 1 (got %d x %d)", who, f, h, w);
        for (int t = 0; t < tiles; ++t) {
            const int32_t *win = tiles_host + ((size_t)f * tiles + t) * 4;
            if (!window_in_frame(win[0], win[1], win[2], win[3], h, w))
                return fail(Y3_ERR_INVALID, "%s: frame %d, tile %d: window %d x %d at (%d, %d) does not lie inside the %d x %d frame", who, f, t,
                            win[2], win[3], win[0], win[1], h, w);
            y3::LetterboxGeom g;
            memcpy(&g, geoms_host + ((size_t)f * tiles + t) * 4, sizeof(g));
            if (!y3::letterbox_geom_fits(g, Hc, Wc))
                return fail(Y3_ERR_INVALID, "%s: frame %d, tile %d: geometry %d x %d at (%d, %d) does not lie inside %d x %d", who, f, t,
                            g.sh, g.sw, g.top, g.left, Hc, Wc);
        }
    }
    const MergeLayout l = merge_layout(frames, tiles, max_boxes);
    if (!workspace_dev || workspace_bytes < l.total) return fail(Y3_ERR_INVALID, "%s: workspace too small (need %zu bytes)", who, l.total);
    if (((uintptr_t)packed_dev & 3) || ((uintptr_t)packed_out_dev & 3) || ((uintptr_t)workspace_dev & 15))
        return fail(Y3_ERR_INVALID, "%s: packed / packed_out not 4-byte or workspace not 16-byte aligned", who);
    char *ws = static_cast<char *>(workspace_dev);
    float *boxes = reinterpret_cast<float *>(ws + l.boxes), *scores = reinterpret_cast<float *>(ws + l.scores);
    int64_t *cls = reinterpret_cast<int64_t *>(ws + l.cls);
    int32_t *sel = reinterpret_cast<int32_t *>(ws + l.sel);
    const int images = frames * tiles, N = tiles * max_boxes;
    const unsigned *packed = static_cast<const unsigned *>(packed_dev);
    for (int i0 = 0; i0 < images; i0 += y3::kMergeTableTiles) {
        const int n = std::min(y3::kMergeTableTiles, images - i0);
        y3::MergeTile entries[y3::kMergeTableTiles];
        for (int i = 0; i < n; ++i) {
            const int gi = i0 + i;
            const int32_t *win = tiles_host + (size_t)gi * 4, *hw = frame_hw_host + (size_t)(gi / tiles) * 2;
            y3::MergeTile &e = entries[i];
            e.y0 = win[0], e.x0 = win[1], e.ch = win[2], e.cw = win[3];
            memcpy(&e.g, geoms_host + (size_t)gi * 4, sizeof(e.g));
            e.h = hw[0], e.w = hw[1];
        }
        const size_t c0 = (size_t)i0 * max_boxes;      // first candidate of the launch
        hipError_t e = y3::launch_merge_tiles(packed + c0 * 7, num_valid_dev + i0, entries, n, max_boxes, Hc, Wc, boxes + c0 * 4, scores + c0,
                                              cls + c0, (hipStream_t)stream);
        if (e != hipSuccess) return fail(Y3_ERR_HIP, "%s launch: %s", who, hipGetErrorString(e));
    }
    return y3::select_and_pack(who, boxes, scores, cls, nullptr, frames, N, max_boxes, nms_mode, iou_threshold, score_threshold, sel,
                               num_valid_out_dev, ws + l.nms, l.nms_bytes, packed_out_dev, stream);
}
Y3_CATCH("y3_merge_tile_detections")

y3_status y3_evaluate_detections(const void *packed_dev, const int32_t *num_valid_dev, int batch, int max_boxes,
                                 const float *gt_boxes_dev, const int32_t *gt_classes_dev, const int32_t *gt_count_dev, int max_gt,
                                 int nclasses, float iou_threshold, const float *score_thresholds_host, int n_thresholds,
                                 int one_class, int64_t *counters_dev, void *stream)
try {
    if (!packed_dev || !num_valid_dev || !gt_boxes_dev || !gt_classes_dev || !gt_count_dev || !score_thresholds_host || !counters_dev)
        return fail(Y3_ERR_INVALID, "y3_evaluate_detections: null pointer");
    if (batch < 1) return fail(Y3_ERR_INVALID, "y3_evaluate_detections: batch must be at least 1 (got %d)", batch);
    if (max_boxes < 1 || max_boxes > y3::kEvalMaxBoxes)
        return fail(Y3_ERR_INVALID, "y3_evaluate_detections: max_boxes must be in [1,%d] (got %d)", y3::kEvalMaxBoxes, max_boxes);
    if (max_gt < 1 || max_gt > y3::kEvalMaxGt)
        return fail(Y3_ERR_INVALID, "y3_evaluate_detections: max_gt must be in [1,%d] (got %d)", y3::kEvalMaxGt, max_gt);
    if (nclasses < 1 || nclasses > y3::kEvalMaxClasses)
        return fail(Y3_ERR_INVALID, "y3_evaluate_detections: nclasses must be in [1,%d] (got %d)", y3::kEvalMaxClasses, nclasses);
    if (n_thresholds < 1 || n_thresholds > y3::kEvalMaxThresholds)
        return fail(Y3_ERR_INVALID, "y3_evaluate_detections: n_thresholds must be in [1,%d] (got %d)", y3::kEvalMaxThresholds, n_thresholds);
    if (((uintptr_t)packed_dev & 3) || ((uintptr_t)gt_boxes_dev & 3) || ((uintptr_t)counters_dev & 7))
        return fail(Y3_ERR_INVALID, "y3_evaluate_detections: packed / gt_boxes not 4-byte or counters not 8-byte aligned");
    y3::EvalThresholds thr{};
    for (int t = 0; t < n_thresholds; ++t) thr.s[t] = score_thresholds_host[t];
    hipError_t e = y3::launch_evaluate(packed_dev, num_valid_dev, batch, max_boxes, gt_boxes_dev, gt_classes_dev, gt_count_dev, max_gt,
                                       nclasses, iou_threshold, thr, n_thresholds, one_class != 0, counters_dev, (hipStream_t)stream);
    if (e != hipSuccess) return fail(Y3_ERR_HIP, "y3_evaluate_detections launch: %s", hipGetErrorString(e));
    return Y3_OK;
}
Y3_CATCH("y3_evaluate_detections")

y3_status y3_match_detections(const void *packed_dev, const int32_t *num_valid_dev, int batch, int max_boxes,
                              const float *gt_boxes_dev, const int32_t *gt_classes_dev, const int32_t *gt_count_dev, int max_gt,
                              int nclasses, const float *iou_thresholds_host, int n_iou, int one_class, uint32_t *records_dev,
                              int64_t *gt_totals_dev, void *stream)
try {
    if (!packed_dev || !num_valid_dev || !gt_boxes_dev || !gt_classes_dev || !gt_count_dev || !iou_thresholds_host || !records_dev ||
        !gt_totals_dev)
        return fail(Y3_ERR_INVALID, "y3_match_detections: null pointer");
    if (batch < 1) return fail(Y3_ERR_INVALID, "y3_match_detections: batch must be at least 1 (got %d)", batch);
    if (max_boxes < 1 || max_boxes > y3::kEvalMaxBoxes)
        return fail(Y3_ERR_INVALID, "y3_match_detections: max_boxes must be in [1,%d] (got %d)", y3::kEvalMaxBoxes, max_boxes);
    if (max_gt < 1 || max_gt > y3::kEvalMaxGt)
        return fail(Y3_ERR_INVALID, "y3_match_detections: max_gt must be in [1,%d] (got %d)", y3::kEvalMaxGt, max_gt);
    if (nclasses < 1 || nclasses > y3::kEvalMaxClasses)
        return fail(Y3_ERR_INVALID, "y3_match_detections: nclasses must be in [1,%d] (got %d)", y3::kEvalMaxClasses, nclasses);
    if (n_iou < 1 || n_iou > y3::kEvalMaxThresholds)
        return fail(Y3_ERR_INVALID, "y3_match_detections: n_iou must be in [1,%d] (got %d)", y3::kEvalMaxThresholds, n_iou);
    y3::EvalThresholds thr{};
    for (int k = 0; k < n_iou; ++k) {
        if (!std::isfinite(iou_thresholds_host[k]))
            return fail(Y3_ERR_INVALID, "y3_match_detections: iou_thresholds[%d] is not finite", k);
        thr.s[k] = iou_thresholds_host[k];
    }
    if (((uintptr_t)packed_dev & 3) || ((uintptr_t)gt_boxes_dev & 3) || ((uintptr_t)records_dev & 7) || ((uintptr_t)gt_totals_dev & 7))
        return fail(Y3_ERR_INVALID, "y3_match_detections: packed / gt_boxes not 4-byte or records / gt_totals not 8-byte aligned");
    hipError_t e = y3::launch_ap_match(packed_dev, num_valid_dev, batch, max_boxes, gt_boxes_dev, gt_classes_dev, gt_count_dev, max_gt,
                                       nclasses, thr, n_iou, one_class != 0, records_dev, gt_totals_dev, (hipStream_t)stream);
    if (e != hipSuccess) return fail(Y3_ERR_HIP, "y3_match_detections launch: %s", hipGetErrorString(e));
    return Y3_OK;
}
Y3_CATCH("y3_match_detections")

// ------------------------------------------------------------------------------------------ validation loss
namespace {
// The checks and the by-value geometry the two loss entries share: grid sizes, first decode row per scale, anchors.
y3_status loss_geometry(const char *who, const int32_t *grid_sizes, const float *anchors_host, int batch, int max_gt, int nclasses,
                        y3::LossGeom *geo)
{
    if (!grid_sizes || !anchors_host) return fail(Y3_ERR_INVALID, "%s: null pointer", who);
    if (batch < 1) return fail(Y3_ERR_INVALID, "%s: batch must be at least 1 (got %d)", who, batch);
    if (max_gt < 1 || max_gt > y3::kEvalMaxGt) return fail(Y3_ERR_INVALID, "%s: max_gt must be in [1,%d] (got %d)", who, y3::kEvalMaxGt, max_gt);
    if (nclasses < 1 || nclasses > y3::kEvalMaxClasses)
        return fail(Y3_ERR_INVALID, "%s: nclasses must be in [1,%d] (got %d)", who, y3::kEvalMaxClasses, nclasses);
    int off = 0;
    for (int s = 0; s < 3; ++s) {
        if (grid_sizes[s] < 1 || grid_sizes[s] > y3::kLossMaxGrid)
            return fail(Y3_ERR_INVALID, "%s: grid_sizes[%d] must be in [1,%d] (got %d)", who, s, y3::kLossMaxGrid, grid_sizes[s]);
        geo->g[s] = grid_sizes[s];
        geo->off[s] = off;
        off += 3 * grid_sizes[s] * grid_sizes[s];
        for (int a = 0; a < 3; ++a) {
            geo->anchors[s][a][0] = anchors_host[(s * 3 + a) * 2 + 0];
            geo->anchors[s][a][1] = anchors_host[(s * 3 + a) * 2 + 1];
        }
    }
    return Y3_OK;
}
}  // namespace

y3_status y3_yolo_assign_targets(const float *gt_boxes_dev, const int32_t *gt_classes_dev, const int32_t *gt_count_dev, int batch,
                                 int max_gt, int nclasses, const int32_t grid_sizes[3], const float *anchors_host,
                                 int32_t *cells_dev, void *stream)
try {
    if (!gt_boxes_dev || !gt_classes_dev || !gt_count_dev || !cells_dev)
        return fail(Y3_ERR_INVALID, "y3_yolo_assign_targets: null pointer");
    y3::LossGeom geo{};
    y3_status st = loss_geometry("y3_yolo_assign_targets", grid_sizes, anchors_host, batch, max_gt, nclasses, &geo);
    if (st != Y3_OK) return st;
    if (((uintptr_t)gt_boxes_dev & 3) || ((uintptr_t)gt_classes_dev & 3) || ((uintptr_t)gt_count_dev & 3) || ((uintptr_t)cells_dev & 3))
        return fail(Y3_ERR_INVALID, "y3_yolo_assign_targets: a device pointer is not 4-byte aligned");
    hipError_t e = y3::launch_assign_targets(gt_boxes_dev, gt_classes_dev, gt_count_dev, batch, max_gt, nclasses, geo, cells_dev,
                                             (hipStream_t)stream);
    if (e != hipSuccess) return fail(Y3_ERR_HIP, "y3_yolo_assign_targets launch: %s", hipGetErrorString(e));
    return Y3_OK;
}
Y3_CATCH("y3_yolo_assign_targets")

y3_status y3_yolo_loss(const float *const grids_dev[3], const int32_t grid_sizes[3], int batch, int nclasses,
                       const float *anchors_host, const float *gt_boxes_dev, const int32_t *gt_classes_dev,
                       const int32_t *cells_dev, int max_gt, double *loss_dev, void *stream)
try {
    if (!grids_dev || !gt_boxes_dev || !gt_classes_dev || !cells_dev || !loss_dev)
        return fail(Y3_ERR_INVALID, "y3_yolo_loss: null pointer");
    y3::LossGeom geo{};
    y3_status st = loss_geometry("y3_yolo_loss", grid_sizes, anchors_host, batch, max_gt, nclasses, &geo);
    if (st != Y3_OK) return st;
    y3::LossGrids grids{};
    for (int s = 0; s < 3; ++s) {
        if (!grids_dev[s] || ((uintptr_t)grids_dev[s] & 3))
            return fail(Y3_ERR_INVALID, "y3_yolo_loss: grid %d null or not 4-byte aligned", s);
        grids.p[s] = grids_dev[s];
    }
    if (((uintptr_t)gt_boxes_dev & 3) || ((uintptr_t)gt_classes_dev & 3) || ((uintptr_t)cells_dev & 3) || ((uintptr_t)loss_dev & 7))
        return fail(Y3_ERR_INVALID, "y3_yolo_loss: gt_boxes / gt_classes / cells not 4-byte or loss not 8-byte aligned");
    hipError_t e = y3::launch_yolo_loss(grids, geo, batch, nclasses, gt_boxes_dev, gt_classes_dev, cells_dev, max_gt, loss_dev,
                                        (hipStream_t)stream);
    if (e != hipSuccess) return fail(Y3_ERR_HIP, "y3_yolo_loss launch: %s", hipGetErrorString(e));
    return Y3_OK;
}
Y3_CATCH("y3_yolo_loss")

// ------------------------------------------------------------------------------------------ TFRecord checksum
uint32_t y3_crc32c(const void *data_host, size_t nbytes)
{
    // slicing-by-8 over the reflected Castagnoli polynomial
    static uint32_t T[8][256];
    static bool ready = [] {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0x82F63B78u & (0u - (c & 1u)));
            T[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; ++i)
            for (int t = 1; t < 8; ++t) T[t][i] = (T[t - 1][i] >> 8) ^ T[0][T[t - 1][i] & 0xFF];
        return true;
    }();
    (void)ready;
    const unsigned char *p = static_cast<const unsigned char *>(data_host);
    uint32_t c = 0xFFFFFFFFu;
    while (nbytes >= 8) {
        uint32_t lo, hi;
        memcpy(&lo, p, 4);
        memcpy(&hi, p + 4, 4);
        lo ^= c;
        c = T[7][lo & 0xFF] ^ T[6][(lo >> 8) & 0xFF] ^ T[5][(lo >> 16) & 0xFF] ^ T[4][lo >> 24] ^ T[3][hi & 0xFF] ^
            T[2][(hi >> 8) & 0xFF] ^ T[1][(hi >> 16) & 0xFF] ^ T[0][hi >> 24];
        p += 8;
        nbytes -= 8;
    }
    while (nbytes--) c = (c >> 8) ^ T[0][(c ^ *p++) & 0xFF];
    return c ^ 0xFFFFFFFFu;
}

// ------------------------------------------------------------------------------------------ decode entry points
y3_status y3_yolo_decode_hw(const float *const grids_dev[3], const int32_t grid_hw[3][2], int batch, int nclasses,
                            const float *anchors_host, float *bboxes_dev, float *conf_dev, float *probs_dev, void *stream)
try {
    return yolo_decode_hw("y3_yolo_decode_hw", grids_dev, grid_hw, 3, batch, nclasses, anchors_host, bboxes_dev, conf_dev, probs_dev, stream);
}
Y3_CATCH("y3_yolo_decode_hw")

y3_status y3_yolo_decode_hw_n(const float *const *grids_dev, const int32_t (*grid_hw)[2], int n_scales, int batch, int nclasses,
                              const float *anchors_host, float *bboxes_dev, float *conf_dev, float *probs_dev, void *stream)
try {
    return yolo_decode_hw("y3_yolo_decode_hw_n", grids_dev, grid_hw, n_scales, batch, nclasses, anchors_host, bboxes_dev, conf_dev, probs_dev, stream);
}
Y3_CATCH("y3_yolo_decode_hw_n")

y3_status y3_yolo_decode_scores_hw_n(const float *const *grids_dev, const int32_t (*grid_hw)[2], int n_scales, int batch, int nclasses,
                                     const float *anchors_host, float *bboxes_dev, int64_t *class_idx_dev, float *scores_dev,
                                     void *stream)
try {
    return y3::decode_scores_hw("y3_yolo_decode_scores_hw_n", grids_dev, grid_hw, n_scales, batch, nclasses, anchors_host, bboxes_dev, class_idx_dev, scores_dev, stream);
}
Y3_CATCH("y3_yolo_decode_scores_hw_n")

y3_status y3_maxpool2x2(const void *src_dev, void *dst_dev, int batch, int height, int width, int channels, int stride, int dtype,
                        void *stream)
try {
    const char *who = "y3_maxpool2x2";
    if (!src_dev || !dst_dev || batch < 1 || height < 1 || width < 1 || channels < 1) return fail(Y3_ERR_INVALID, "%s: bad argument", who);
    if (dtype != Y3_DTYPE_F32 && dtype != Y3_DTYPE_BF16 && dtype != Y3_DTYPE_F16 && dtype != Y3_DTYPE_I8)
        return fail(Y3_ERR_INVALID, "%s: dtype must be Y3_DTYPE_F32, Y3_DTYPE_BF16, Y3_DTYPE_F16 or Y3_DTYPE_I8 (got %d)", who, dtype);
    if (stride != 1 && stride != 2) return fail(Y3_ERR_INVALID, "%s: stride must be 1 or 2 (got %d)", who, stride);
    if (stride == 2 && ((height | width) & 1)) return fail(Y3_ERR_INVALID, "%s: a stride-2 pool needs even extents (got %d x %d)", who, height, width);
    const int eb = dtype == Y3_DTYPE_F32 ? 4 : dtype == Y3_DTYPE_I8 ? 1 : 2;
    if (((long long)channels * eb) % 16) return fail(Y3_ERR_INVALID, "%s: %d channels of %d bytes are no multiple of 16 bytes", who, channels, eb);
    if (((uintptr_t)src_dev & 15) || ((uintptr_t)dst_dev & 15)) return fail(Y3_ERR_INVALID, "%s: src / dst not 16-byte aligned", who);
    if ((long long)batch * (height / stride) > 0x7fffffffll || (long long)(width / stride) * channels * eb / 16 > 0x00ffffffll)
        return fail(Y3_ERR_INVALID, "%s: batch * output rows must stay below 2^31 and an output row below 2^28 bytes", who);
    hipError_t e = y3::launch_maxpool2x2(src_dev, dst_dev, batch, height, width, channels, stride, dtype, (hipStream_t)stream);
    if (e != hipSuccess) return fail(Y3_ERR_HIP, "%s launch: %s", who, hipGetErrorString(e));
    return Y3_OK;
}
Y3_CATCH("y3_maxpool2x2")

y3_status y3_yolo_decode_scores_hw(const float *const grids_dev[3], const int32_t grid_hw[3][2], int batch, int nclasses,
                                   const float *anchors_host, float *bboxes_dev, int64_t *class_idx_dev,
                                   float *scores_dev, void *stream)
try {
    return y3::decode_scores_hw("y3_yolo_decode_scores_hw", grids_dev, grid_hw, 3, batch, nclasses, anchors_host, bboxes_dev, class_idx_dev, scores_dev, stream);
}
Y3_CATCH("y3_yolo_decode_scores_hw")

y3_status y3_yolo_decode(const float *const grids_dev[3], const int32_t grid_sizes[3], int batch, int nclasses,
                         const float *anchors_host, float *bboxes_dev, float *conf_dev, float *probs_dev, void *stream)
try {
    if (!conf_dev || !probs_dev) return fail(Y3_ERR_INVALID, "y3_yolo_decode: null output");
    if (!grid_sizes) return fail(Y3_ERR_INVALID, "y3_yolo_decode: bad argument");
    const int32_t hw[3][2] = {{grid_sizes[0], grid_sizes[0]}, {grid_sizes[1], grid_sizes[1]}, {grid_sizes[2], grid_sizes[2]}};
    return yolo_decode_hw("y3_yolo_decode", grids_dev, hw, 3, batch, nclasses, anchors_host, bboxes_dev, conf_dev, probs_dev, stream);
}
Y3_CATCH("y3_yolo_decode")

y3_status y3_yolo_decode_scores(const float *const grids_dev[3], const int32_t grid_sizes[3], int batch, int nclasses,
                                const float *anchors_host, float *bboxes_dev, int64_t *class_idx_dev,
                                float *scores_dev, void *stream)
try {
    if (!class_idx_dev || !scores_dev) return fail(Y3_ERR_INVALID, "y3_yolo_decode_scores: null output");
    if (!grid_sizes) return fail(Y3_ERR_INVALID, "y3_yolo_decode_scores: bad argument");
    const int32_t hw[3][2] = {{grid_sizes[0], grid_sizes[0]}, {grid_sizes[1], grid_sizes[1]}, {grid_sizes[2], grid_sizes[2]}};
    return y3::decode_scores_hw("y3_yolo_decode_scores", grids_dev, hw, 3, batch, nclasses, anchors_host, bboxes_dev, class_idx_dev, scores_dev, stream);
}
Y3_CATCH("y3_yolo_decode_scores")

size_t y3_decode_candidates_workspace_bytes_n(const int32_t (*grid_hw)[2], int n_scales, int batch, int nclasses)
{
    if (!grid_hw || batch < 1 || nclasses < 1) return 0;
    const long long N = grid_boxes(grid_hw, n_scales);
    if (N <= 0 || (long long)batch * N > 0x7fffffffll) return 0;
    return (size_t)batch * (size_t)N * sizeof(int32_t);
}

size_t y3_decode_candidates_workspace_bytes(const int32_t grid_hw[3][2], int batch, int nclasses)
{
    return y3_decode_candidates_workspace_bytes_n(grid_hw, 3, batch, nclasses);
}

y3_status y3_yolo_decode_candidates_hw_n(const float *const *grids_dev, const int32_t (*grid_hw)[2], int n_scales, int batch, int nclasses,
                                         const float *anchors_host, float score_threshold, int capacity, float *cand_boxes_dev,
                                         int64_t *cand_cls_dev, float *cand_scores_dev, int32_t *cand_src_dev, int32_t *totals_dev,
                                         void *workspace_dev, size_t workspace_bytes, void *stream)
try {
    return y3::decode_candidates_hw("y3_yolo_decode_candidates_hw_n", grids_dev, grid_hw, n_scales, batch, nclasses, anchors_host, score_threshold,
                                    capacity, cand_boxes_dev, cand_cls_dev, cand_scores_dev, cand_src_dev, totals_dev, workspace_dev,
                                    workspace_bytes, stream);
}
Y3_CATCH("y3_yolo_decode_candidates_hw_n")

y3_status y3_yolo_decode_candidates_hw(const float *const grids_dev[3], const int32_t grid_hw[3][2], int batch, int nclasses,
                                       const float *anchors_host, float score_threshold, int capacity, float *cand_boxes_dev,
                                       int64_t *cand_cls_dev, float *cand_scores_dev, int32_t *cand_src_dev, int32_t *totals_dev,
                                       void *workspace_dev, size_t workspace_bytes, void *stream)
try {
    return y3::decode_candidates_hw("y3_yolo_decode_candidates_hw", grids_dev, grid_hw, 3, batch, nclasses, anchors_host, score_threshold, capacity,
                                    cand_boxes_dev, cand_cls_dev, cand_scores_dev, cand_src_dev, totals_dev, workspace_dev, workspace_bytes, stream);
}
Y3_CATCH("y3_yolo_decode_candidates_hw")

y3_status y3_class_candidates(const float *bboxes_dev, const float *conf_dev, const float *probs_dev, int batch, int n, int nclasses,
                              float score_threshold, int capacity, float *cand_boxes_dev, int64_t *cand_cls_dev, float *cand_scores_dev,
                              int32_t *cand_src_dev, int32_t *totals_dev, void *workspace_dev, size_t workspace_bytes, void *stream)
try {
    const char *who = "y3_class_candidates";
    if (!bboxes_dev || !conf_dev || !probs_dev || !cand_boxes_dev || !cand_cls_dev || !cand_scores_dev || !cand_src_dev || !totals_dev)
        return fail(Y3_ERR_INVALID, "%s: null pointer", who);
    if (batch < 1 || n < 1 || capacity < 1 || nclasses < 1)
        return fail(Y3_ERR_INVALID, "%s: batch, n, capacity and nclasses must be at least 1 (got %d, %d, %d, %d)", who, batch, n, capacity, nclasses);
    if ((long long)batch * capacity > 0x7fffffffll || (long long)n * nclasses > 0x7fffffffll || (long long)batch * n > 0x7fffffffll)
        return fail(Y3_ERR_INVALID, "%s: batch * capacity, n * nclasses and batch * n must stay below 2^31", who);
    if (((uintptr_t)bboxes_dev & 15) || ((uintptr_t)cand_boxes_dev & 15)) return fail(Y3_ERR_INVALID, "%s: bboxes / cand_boxes not 16-byte aligned", who);
    if (((uintptr_t)cand_cls_dev & 7) || ((uintptr_t)conf_dev & 3) || ((uintptr_t)probs_dev & 3) || ((uintptr_t)cand_scores_dev & 3) ||
        ((uintptr_t)cand_src_dev & 3) || ((uintptr_t)totals_dev & 3))
        return fail(Y3_ERR_INVALID, "%s: cand_cls not 8-byte or a float / int32 pointer not 4-byte aligned", who);
    const size_t need = (size_t)batch * (size_t)n * sizeof(int32_t);
    if (!workspace_dev || workspace_bytes < need || ((uintptr_t)workspace_dev & 3))
        return fail(Y3_ERR_INVALID, "%s: workspace too small or not 4-byte aligned (need %zu bytes)", who, need);
    hipError_t e = y3::launch_class_candidates(bboxes_dev, conf_dev, probs_dev, batch, n, nclasses, score_threshold, capacity, cand_boxes_dev,
                                               cand_cls_dev, cand_scores_dev, cand_src_dev, totals_dev, static_cast<int32_t *>(workspace_dev),
                                               (hipStream_t)stream);
    if (e != hipSuccess) return fail(Y3_ERR_HIP, "%s launch: %s", who, hipGetErrorString(e));
    return Y3_OK;
}
Y3_CATCH("y3_class_candidates")

y3_status y3_candidate_sources(void *packed_dev, const int32_t *num_valid_dev, const int32_t *cand_src_dev, int batch, int capacity,
                               int max_boxes, void *stream)
try {
    if (!packed_dev || !num_valid_dev || !cand_src_dev) return fail(Y3_ERR_INVALID, "y3_candidate_sources: null pointer");
    if (batch < 1 || capacity < 1 || max_boxes < 1 || (long long)batch * capacity > 0x7fffffffll || (long long)batch * max_boxes > 0x7fffffffll)
        return fail(Y3_ERR_INVALID, "y3_candidate_sources: batch, capacity and max_boxes must be at least 1, batch * capacity and batch * max_boxes below 2^31");
    if (((uintptr_t)packed_dev & 3) || ((uintptr_t)num_valid_dev & 3) || ((uintptr_t)cand_src_dev & 3))
        return fail(Y3_ERR_INVALID, "y3_candidate_sources: a device pointer is not 4-byte aligned");
    hipError_t e = y3::launch_candidate_sources(packed_dev, num_valid_dev, cand_src_dev, batch, capacity, max_boxes, (hipStream_t)stream);
    if (e != hipSuccess) return fail(Y3_ERR_HIP, "y3_candidate_sources launch: %s", hipGetErrorString(e));
    return Y3_OK;
}
Y3_CATCH("y3_candidate_sources")

y3_status y3_class_scores(const float *conf_dev, const float *probs_dev, int batch, int n, int nclasses,
                          int64_t *class_idx_dev, float *scores_dev, void *stream)
try {
    if (!conf_dev || !probs_dev || !class_idx_dev || !scores_dev || batch <= 0 || n <= 0 || nclasses <= 0)
        return fail(Y3_ERR_INVALID, "y3_class_scores: bad argument");
    hipError_t e = y3::launch_class_scores(conf_dev, probs_dev, (size_t)batch * n, nclasses, class_idx_dev, scores_dev,
                                           (hipStream_t)stream);
    if (e != hipSuccess) return fail(Y3_ERR_HIP, "y3_class_scores launch: %s", hipGetErrorString(e));
    return Y3_OK;
}
Y3_CATCH("y3_class_scores")

size_t y3_nms_workspace_bytes(int batch, int n) { return (batch > 0 && n > 0) ? y3::nms_workspace_bytes(batch, n) : 0; }
size_t y3_nms_per_class_workspace_bytes(int batch, int n) { return (batch > 0 && n > 0) ? y3::nms_per_class_workspace_bytes(batch, n) : 0; }

// y3_nms_padded (class_idx_dev null) and y3_nms_padded_per_class: the argument checks both share, then the one launch
static y3_status nms_padded(const char *who, const float *bboxes_dev, const float *scores_dev, const int64_t *class_idx_dev, int batch,
                            int n, int max_output_size, float iou_threshold, float score_threshold, int32_t *selected_idx_dev,
                            int32_t *num_valid_dev, void *workspace_dev, size_t workspace_bytes, void *stream)
{
    if (!bboxes_dev || !scores_dev || !selected_idx_dev || !num_valid_dev || batch <= 0 || n <= 0)
        return fail(Y3_ERR_INVALID, "%s: bad argument", who);
    if (max_output_size <= 0 || max_output_size > 1024)
        return fail(Y3_ERR_INVALID, "%s: max_output_size must be in [1,1024]", who);
    if ((uintptr_t)bboxes_dev & 15) return fail(Y3_ERR_INVALID, "%s: bboxes not 16-byte aligned", who);
    if (class_idx_dev && !(iou_threshold > 0.0f))
        return fail(Y3_ERR_INVALID, "%s: iou_threshold must be > 0 (iou_threshold <= 0 is the tile quirk of the class-agnostic rule)", who);
    if (!(iou_threshold > 0.0f) && score_threshold < 0.0f)
        return fail(Y3_ERR_INVALID, "%s: iou_threshold <= 0 together with score_threshold < 0 is not supported", who);
    const size_t need = class_idx_dev ? y3::nms_per_class_workspace_bytes(batch, n) : y3::nms_workspace_bytes(batch, n);
    if (!workspace_dev || workspace_bytes < need) return fail(Y3_ERR_INVALID, "%s: workspace too small (need %zu bytes)", who, need);
    hipError_t e = y3::launch_nms(bboxes_dev, scores_dev, class_idx_dev, batch, n, max_output_size, iou_threshold, score_threshold,
                                  selected_idx_dev, num_valid_dev, workspace_dev, (hipStream_t)stream);
    if (e != hipSuccess) return fail(Y3_ERR_HIP, "%s launch: %s", who, hipGetErrorString(e));
    return Y3_OK;
}

y3_status y3_nms_padded(const float *bboxes_dev, const float *scores_dev, int batch, int n, int max_output_size,
                        float iou_threshold, float score_threshold, int32_t *selected_idx_dev,
                        int32_t *num_valid_dev, void *workspace_dev, size_t workspace_bytes, void *stream)
try {
    return nms_padded("y3_nms_padded", bboxes_dev, scores_dev, nullptr, batch, n, max_output_size, iou_threshold, score_threshold,
                      selected_idx_dev, num_valid_dev, workspace_dev, workspace_bytes, stream);
}
Y3_CATCH("y3_nms_padded")

y3_status y3_nms_padded_per_class(const float *bboxes_dev, const float *scores_dev, const int64_t *class_idx_dev, int batch, int n,
                                  int max_output_size, float iou_threshold, float score_threshold, int32_t *selected_idx_dev,
                                  int32_t *num_valid_dev, void *workspace_dev, size_t workspace_bytes, void *stream)
try {
    if (!class_idx_dev) return fail(Y3_ERR_INVALID, "y3_nms_padded_per_class: bad argument");
    return nms_padded("y3_nms_padded_per_class", bboxes_dev, scores_dev, class_idx_dev, batch, n, max_output_size, iou_threshold,
                      score_threshold, selected_idx_dev, num_valid_dev, workspace_dev, workspace_bytes, stream);
}
Y3_CATCH("y3_nms_padded_per_class")

y3_status y3_pack_detections(const float *bboxes_dev, const int64_t *class_idx_dev, const float *scores_dev,
                             const int32_t *selected_idx_dev, const int32_t *num_valid_dev, int batch, int n,
                             int max_out, void *packed_dev, void *stream)
try {
    if (!bboxes_dev || !class_idx_dev || !scores_dev || !selected_idx_dev || !num_valid_dev || !packed_dev ||
        batch <= 0 || n <= 0 || max_out <= 0)
        return fail(Y3_ERR_INVALID, "y3_pack_detections: bad argument");
    hipError_t e = y3::launch_pack(bboxes_dev, class_idx_dev, scores_dev, selected_idx_dev, num_valid_dev, batch, n,
                                   max_out, packed_dev, (hipStream_t)stream);
    if (e != hipSuccess) return fail(Y3_ERR_HIP, "y3_pack_detections launch: %s", hipGetErrorString(e));
    return Y3_OK;
}
Y3_CATCH("y3_pack_detections")

}  // extern "C"

// ------------------------------------------------------------------------------------------ the detection tail (y3_host.h)
y3_status y3::select_check(const char *who, int nms_mode, float iou_threshold, float score_threshold)
{
    if (nms_mode == Y3_NMS_PER_CLASS && !(iou_threshold > 0.0f))
        return fail(Y3_ERR_INVALID, "%s: iou_threshold must be > 0 with Y3_NMS_PER_CLASS", who);
    if (!(iou_threshold > 0.0f) && score_threshold < 0.0f)
        return fail(Y3_ERR_INVALID, "%s: iou_threshold <= 0 together with score_threshold < 0 is not supported", who);
    return Y3_OK;
}

y3_status y3::select_and_pack(const char *who, const float *boxes, const float *scores, const int64_t *cls, const int32_t *cand_src, int batch,
                              int n, int max_boxes, int nms_mode, float iou_threshold, float score_threshold, int32_t *sel, int32_t *num_valid,
                              void *ws, size_t ws_bytes, void *packed, void *stream)
{
    y3_status st = nms_padded(who, boxes, scores, nms_mode == Y3_NMS_PER_CLASS ? cls : nullptr, batch, n, max_boxes, iou_threshold, score_threshold,
                              sel, num_valid, ws, ws_bytes, stream);
    if (st != Y3_OK) return st;
    hipError_t e = y3::launch_pack(boxes, cls, scores, sel, num_valid, batch, n, max_boxes, packed, (hipStream_t)stream);
    if (e == hipSuccess && cand_src) e = y3::launch_candidate_sources(packed, num_valid, cand_src, batch, n, max_boxes, (hipStream_t)stream);
    if (e != hipSuccess) return fail(Y3_ERR_HIP, "%s: pack launch: %s", who, hipGetErrorString(e));
    return Y3_OK;
}
