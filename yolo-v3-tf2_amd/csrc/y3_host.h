// Host-only internals of liby3hip.so, shared by y3_net.cpp, y3_plan.cpp, y3_forward.cpp, y3_ops.cpp and comm.cpp: the error plumbing of
// the C ABI, the net object, and what crosses those files.  No .hip file includes it (the kernels see y3_kernels.h only).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/y3.h"
#include "y3_kernels.h"

namespace y3 {
// record the message as this thread's last error and return `code` (a fixed thread-local buffer: reporting allocates nothing)
int fail_msg(int code, const char *fmt, ...) noexcept;
// The exception barrier of the C ABI.  Every extern "C" entry point that can reach an allocation (std::vector, new, std::string)
// is a function-try-block ending in Y3_CATCH: a C++ exception becomes a status + message instead of crossing the boundary and
// terminating the host process (a ctypes / cgo / JNI caller has no handler for it).
int on_exception(const char *who) noexcept;
// Test hook (tests/test_abi.py): Y3_TEST_FAIL_ALLOC=1 makes the object allocations of y3_net_create / y3_comm_init_rank fail the
// way operator new does; read on every call so that a test can switch it on and off inside one process.
bool test_fail_alloc() noexcept;
}  // namespace y3

#define Y3_CATCH(who) catch (...) { return y3::on_exception(who); }

constexpr auto fail = y3::fail_msg;

#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail(e_ == hipErrorOutOfMemory ? Y3_ERR_OOM : Y3_ERR_HIP, "%s: %s", #expr,     \
                        hipGetErrorString(e_));                                                   \
    } while (0)

// Enter the net's device for the duration of a call and give the caller its own current device back on every return path (a
// process driving several GPUs -- PyTorch with nets on different devices -- must not find its current device changed).
struct DeviceGuard {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev)
    {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) err = hipSetDevice(dev); else if (err == hipSuccess) prev = -1;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};
#define Y3_ENTER_DEVICE(net_)                                                                      \
    DeviceGuard dev_guard_((net_)->device);                                                        \
    if (dev_guard_.err != hipSuccess) return fail(Y3_ERR_HIP, "hipSetDevice(%d): %s", (net_)->device, hipGetErrorString(dev_guard_.err))

struct ConvSlot {
    y3_conv_desc d{};
    bool loaded = false;
    bool first_layer = false;  // Cin == 3 direct kernel
    int cout_pad = 0;
    int K = 0;
    int tile = -1;             // -1: choose by heuristic at plan time
    int split_req = -1;        // y3_net_set_split_k: -1 the heuristic (low-latency plans only), 1 off, 2..16 forced
    int split_req_bf16 = -1;   // y3_net_set_split_k_bf16: as split_req, for bf16 plans
    int split_req_f16 = -1;    // y3_net_set_split_k_f16: as split_req, for fp16 plans
    int split_req_i8 = -1;     // y3_net_set_split_k_i8: as split_req, for the int8 convs of an int8 plan
    int split_k = 1;           // K slices in force in the current plan, decided by resolve_splits from plan-time quantities only (1: the unsplit launch)
    int tile_bf16 = -1;        // the 16-bit plans' forced tile: bf16 and fp16 plans share the tile table (y3_net_set_tile_bf16)
    int tile_x3 = -1;
    int cout_pad64 = 0;        // Cout rounded up to 64 (the three-plane kernel has no 32-wide N tile)
    void *wx3_dev = nullptr;   // packed [CoutPad64][3 planes][K] bf16 (hi, mid, lo of the fp32 weights)
    int tile_x2 = -1;
    bool x2_ok = true;         // false: a BN-scaled weight is outside the fp16 range, the two-plane mode cannot be planned
    // packed [CoutPad64][2 planes][K] fp16: h, l' = (w - h) * 2^11 of the BN-scaled weights, every output channel n divided by 2^e_n first
    // (its largest magnitude in [1, 2); e_n = 0 for an all-zero channel), and scale_x2_dev[n] = 2^e_n, which the kernel's epilogue applies
    void *wx2_dev = nullptr;
    float *scale_x2_dev = nullptr;   // [CoutPad64]
    void *w_dev = nullptr;     // packed [CoutPad][K] fp32 (or HWIO for the first layer)
    float *w0stem_dev = nullptr;   // first layer only: [28][Cout] = HWIO rows x BN scale, row 27 zero (fused stem kernel, fp32)
    float *w0raw_dev = nullptr;    // first layer only: the same without the scale (fused stem kernel, bf16 mode)
    // first layer only, fused stem kernel of fp16 plans: w0raw_dev with every output channel n divided by 2^e_n (its largest magnitude in
    // [1, 2); e_n = 0 for an all-zero channel), and the conv0 scale of that kernel alone, scale * 2^e_n (scale_dev stays conv_first's)
    float *w0norm_dev = nullptr;
    float *scale0norm_dev = nullptr;
    // fused tiny stem (conv_tiny_stem.hip), the kernel's own copies at the real widths.  First layer: w0tiny_dev [27][16], the HWIO rows of
    // output channels 0..15, unscaled (scale_dev / shift_dev carry their scale and shift in their first 16 entries), and tiny_pad_zero: output
    // channels 16..31 have scale 0 and shift 0, that is, they are the lowering's zero pad channels.  A 3x3 conv 32 -> 32: w1tiny_*_dev
    // [144][32], row tap * 16 + c from input channels c < 16, unscaled, in fp32, bf16 and fp16
    float *w0tiny_dev = nullptr;
    bool tiny_pad_zero = false;
    void *w1tiny_dev = nullptr, *w1tiny_bf_dev = nullptr, *w1tiny_f16_dev = nullptr;
    void *wbf_dev = nullptr;   // same, bf16 (not for the first layer)
    void *wf16_dev = nullptr;  // same, IEEE fp16 rounded to nearest even on the host (Y3_DTYPE_F16 plans; not for the first layer)
    float *scale_dev = nullptr;
    float *shift_dev = nullptr;
    // int8 plans (Y3_DTYPE_I8; not for the first layer): the raw weights quantised per output channel, packed [CoutPad64][K] int8, with
    // their scales s_w[c] and the BN scale on the host; sc_i8_dev = (s_in * s_w[c]) * bn_scale[c], formed when the plan knows s_in
    void *wi8_dev = nullptr;
    std::vector<float> sw_host, bn_scale_host;   // [CoutPad64]
    float *sc_i8_dev = nullptr;                  // [CoutPad64]
    float q_res = 0.0f, q_inv = 0.0f;            // (at plan time) scale of the int8 shortcut tensor; 1 / scale of the int8 output tensor
    const uint32_t *pos_tab = nullptr;           // (at plan time, fp32 plans) the position table of this 3x3 single-source conv's geometry, else null
    int pos_border = 0;                          // ... and how many of its positions, the table's first, have a tap outside the image
};

struct Op {
    int kind;  // 0 conv, 1 aux
    int index;
};

constexpr int Y3_MAX_LANES = 4;
constexpr int Y3_MAX_OUTPUT_BOXES = 1024;   // upper bound of max_output_size (y3_nms_padded) the detect scratch is sized for

struct y3_net {
    int device = 0;
    int n_cus = 0;                 // compute units of `device`, read once by y3_net_plan (grids of the persistent kernels)
    std::vector<y3_tensor_desc> tensors;
    std::vector<Op> ops;
    std::vector<ConvSlot> convs;
    std::vector<y3_aux_desc> aux;
    int input_tensor = 0;
    int outputs[3] = {0, 0, 0};
    int n_heads = 3;               // how many of them the net has (y3_net_create_heads): 3, or 2 for YOLOv3-tiny
    bool has_pool = false;         // an aux op is a max-pool: fp32, bf16 and fp16 plans, and int8 plans with y3_net_set_pools_i8 (y3_net_plan)
    int nclasses = 0;
    // plan
    int max_batch = 0, height = 0, width = 0, dtype = Y3_DTYPE_F32;   // the planned canvas: height x width (0: no plan)
    int keep_all = 0;              // y3_net_keep_activations: 1: no buffer reuse, every intermediate stays readable after a forward; read by y3_net_plan
    int kept = 0;                  // (at plan time) keep_all as the plan found it: what the arena is, and what every decision of the planned net follows
    int lanes = 1;                 // sub-batches run concurrently on forked streams (y3_net_set_lanes)
    int early_convs = 0;           // y3_net_set_early_chunk: the first early_convs convs run early_chunk images at a time
    int early_chunk = 0;
    int early_ops = 0;             // (at plan time) number of leading ops that form the chunked segment
    int early_step = 0;            // (at plan time) images per chunk of that segment: early_chunk as the plan found it, >= 1 whenever early_ops > 0
    std::vector<char> dense;       // tensor written by the chunked segment: own block, image i at i * image_bytes
    // (non-fp32 modes) output tensors that another op reads, or that a residual / first-layer conv writes: produced in
    // the arena in the mode's own format and converted into the caller's fp32 buffer at the end of the forward
    std::vector<char> staged;
    // per tensor: which of the caller's three fp32 grids a launch writes it into (a net output that is not staged), -1 for every
    // other tensor (all of them before the first plan)
    std::vector<signed char> out_slot;
    // y3_net_detect scratch (grids, decoded boxes / classes / scores, selected indices, NMS workspace): allocated by
    // y3_net_plan for max_batch images and Y3_MAX_OUTPUT_BOXES rows, so y3_net_detect itself only enqueues work
    void *det_buf = nullptr;
    size_t det_bytes = 0;
    int nms_mode = 0;              // y3_net_set_nms_mode: Y3_NMS_AGNOSTIC / Y3_NMS_PER_CLASS, read by y3_net_detect when it enqueues
    int multi_label = 0;           // y3_net_set_multi_label: y3_net_detect enqueues the candidates route; read when it enqueues
    int multi_label_capacity = 0;  // ... with this many candidate slots per image, 0: N of the plan
    int multi_label_batch = 0;     // images of the last multi-label detect enqueued on this plan (where its totals lie: detect_layout of that batch)
    int stem_mode = 1;             // y3_net_set_stem_fusion: 1 = conv0 + conv1 (+ the 1x1 after them) as one kernel when the graph allows it; 2 = conv0 + conv1 only
    bool stem_mode_set = false;    // y3_net_set_stem_fusion was called (the Y3_STEM_MODE tool override then stays out)
    int stem_mode_f16 = 0;         // y3_net_set_stem_fusion_f16: the same three values for Y3_DTYPE_F16 plans, which stem_mode does not act on; off by default
    bool stem_fused = false;       // (at plan time) the first two convs run as the fused stem kernel
    bool stem_conv2 = false;       // ... and the 1x1 conv that follows them (64 -> 32) runs inside it as well (fp32 and bf16 plans)
    int tiny_stem_mode = 0;        // y3_net_set_tiny_stem_fusion: 1 = conv0 + pool 0 + conv1 + pool 1 of YOLOv3-tiny as one kernel when the graph allows it (fp32, bf16, fp16 plans); read by y3_net_plan
    bool tiny_stem_fused = false;  // (at plan time) ops 0..3 run as the fused tiny stem kernel, launched by op 2
    std::vector<char> tiny_inner;  // ... and the tensors inside it (conv0's, pool 0's, conv1's): no launch stores them, they get no arena block
    int xcd_mode = 1;              // y3_net_set_xcd_mode: 0 contiguous tile runs per XCD, 1 XCD-blocked order chosen per conv
    bool low_latency_set = false;  // y3_net_set_low_latency was called (the Y3_LOW_LATENCY tool override then stays out)
    bool low_latency = false;      // y3_net_set_low_latency: every eligible fp32 conv takes y3_choose_split_k
    bool low_latency_bf16 = false; // y3_net_set_low_latency_bf16: every eligible bf16 conv takes y3_choose_split_k
    bool low_latency_f16 = false;  // y3_net_set_low_latency_f16: every eligible fp16 conv takes y3_choose_split_k
    bool low_latency_i8 = false;   // y3_net_set_low_latency_i8: every eligible int8 conv of an int8 plan takes y3_choose_split_k
    void *split_ws = nullptr;      // split-K slabs: split_ws_lanes regions of split_ws_lane bytes, one per lane (lanes run concurrently)
    size_t split_ws_lane = 0;
    int split_ws_lanes = 0;
    int k_chunk = -1;              // y3_net_set_k_chunk: fp32 3x3 convs walk K chunk-major, this many input channels per chunk; 0 tap-major; -1 per-conv default
    // y3_net_set_border_skip: fp32 3x3 convs on batch-minor rows that skip their padding taps; -1 the rule, 0 off, 1 on wherever legal.
    // pos_tabs: one position table per conv geometry of the plan (y3_plan.cpp), on the device, freed with the plan; ConvSlot::pos_tab points into it
    int border_skip = -1;
    struct PosTab { int Ho, Wo, H, W, stride; uint32_t *dev; int border; };   // border: positions with mask9 != 0x1ff, the table's first
    std::vector<PosTab> pos_tabs;
    hipEvent_t fork_ev = nullptr;
    hipStream_t lane_stream[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t join_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<void *> tdev;      // arena pointer per tensor (nullptr: not materialised / external)
    std::vector<size_t> tbytes;    // bytes at max_batch
    std::vector<size_t> tblock;    // size of the arena block the tensor lives in
    std::vector<void *> blocks;    // distinct hipMalloc'ed blocks
    // (batch, lanes) of the last forward enqueued on this plan, 0 before the first: where its images lie in the arena (y3_lane_offset), for
    // y3_net_read_tensor.  The one thing a forward notes in the net it otherwise only reads.
    mutable int last_batch = 0, last_lanes = 0;
    // int8 plans.  act_scale: y3_net_set_act_scales, one fp32 scale per tensor, <= 0 unset (read by y3_net_plan).  i8_first_conv: c*, the
    // first conv slot that runs in int8 (-1: not an int8 plan); the convs before it launch what an fp16 plan launches.  telem: bytes per
    // element of every tensor in the arena (every plan: the mode's; int8 plans: 2 before the cut, 1 behind it).  tq8: the int8 copy of a
    // tensor written before the cut (or handed in) and read behind it (tcross: such a tensor, decided before the arena is placed), image i
    // at i * image elements; tscale: the scales the plan took.
    // pools_i8_mode: y3_net_set_pools_i8, read by y3_net_plan; aux_i8: (at plan time) per aux op, 1 when the plan runs it on int8 tensors
    // behind the cut (a max-pool, an up-sample or a concat whose every source is behind the cut), else the op runs as in an fp16 plan.
    std::vector<float> act_scale;
    int pools_i8_mode = 0;
    bool pools_i8_plan = false;    // (at plan time) pools_i8_mode as the int8 plan in force found it
    std::vector<char> aux_i8;
    int i8_first_conv = -1;
    std::vector<unsigned char> telem;
    std::vector<char> tcross;
    std::vector<void *> tq8;
    std::vector<float> tscale;
};

inline int rows(const y3_net *n, int t) { return n->height / n->tensors[t].div; }
inline int cols(const y3_net *n, int t) { return n->width / n->tensors[t].div; }
inline bool is_output(const y3_net *net, int t)
{
    for (int k = 0; k < net->n_heads; ++k)
        if (t == net->outputs[k]) return true;
    return false;
}

namespace y3 {

// One conv family per plan mode (Y3_DTYPE_*): its tile table (y3_tile_built), the tile a caller forced on a conv, the texts with which
// its setter refuses one (y3_net_set_tile*), and what a launch of the mode takes: weights, chooser, launcher.
struct ConvChoice;
// What a mode needs in order to split K (ConvFamily::split).  The request and the switch stay per mode; ConvSlot::split_k is the plan's.
struct SplitForm {
    bool (*tile)(int);                             // the tile ids with a split form
    hipError_t (*launch)(const ConvArgs &, int tile, bool out_f32, int S, void *ws, size_t ws_bytes, hipStream_t);
    int bk, min_k_tiles;                           // K-tile width of those tiles; the rule leaves a conv of fewer K tiles alone
    int ConvSlot::*req;                            // the caller's request: -1 the rule (low-latency plans only), 1 off, 2..16 forced
    bool y3_net::*low_latency;                     // the switch: every eligible conv takes y3_choose_split_k
    const char *set_split, *set_switch;            // the two setters' names, for their messages
    const char *(*no_form)(int tile);              // refusals: the tile has no split form,
    const char *tiles, *other_plan;                // nor has the tile at the planned rows ("tiles A and B have"), the plan is another mode's,
    int cout_mult;                                 // Cout of a conv storing the mode's own format is no multiple of this
    const char *bad_cout;
};
struct ConvFamily {
    int count;                                     // tile ids are [0, count)
    TileInfo (*info)(int);
    bool (*built)(int);
    int ConvSlot::*tile;                           // forced tile, -1: the chooser's
    int ConvSlot::*cout_pad;                       // padded Cout of the mode's packed weights
    const char *bad, *retired, *misfit;            // refusals: bad argument, retired id (format: the id), tile does not fit the conv
    int resident;                                  // id of the weight-resident kernel, -1: none
    y3_status (*resident_rule)(const y3_net *, const ConvSlot &, int slot);   // its own shape rule
    void *ConvSlot::*w;                            // packed weights [CoutPad][K] values of the mode
    // bytes per value of the mode, in the arena and in a packed weight row (K of them): fp32, bf16, three bf16 planes, two fp16 planes
    int elem_bytes;
    // M: rows of the call; M_plan: rows of the planned batch; arena_out: the launch stores the mode's own format, not an fp32 grid
    int (*choose)(const ConvSlot &, long long M, long long M_plan, bool arena_out);
    hipError_t (*launch)(const ConvArgs &, int tile, bool out_f32, hipStream_t);
    // what the mode adds to the choice once its tile is known (null: nothing)
    void (*refine)(const y3_net *, const ConvSlot &, const ConvArgs &, ConvChoice &);
    // fused stem kernel (null: the mode has none) and the first layer's 28-row weights it reads
    hipError_t (*launch_stem)(const StemArgs &, hipStream_t);
    float *ConvSlot::*w0_stem;
    float *ConvSlot::*scale0_stem;                 // conv0's scale for that kernel (fp16: its weights are normalised per channel)
    int y3_net::*stem_mode;                        // the switch: 0 off, 1 conv0 + conv1 + the 1x1 after them, 2 conv0 + conv1
    const SplitForm *split;                        // null: the mode never splits K
    // fused tiny stem kernel (null: the mode has none) and conv1's [144][32] weights it reads
    hipError_t (*launch_tiny_stem)(const TinyStemArgs &, hipStream_t);
    void *ConvSlot::*w1_tiny;
};
const ConvFamily *conv_family(int dtype);   // null: no such mode
inline const ConvFamily &family_of(const y3_net *net) { return *conv_family(net->dtype); }   // the planned mode's (fp32 before the first plan)
// ... of conv `slot`: an int8 plan runs the convs before its cut as an fp16 plan does
inline bool conv_is_i8(const y3_net *net, int slot) { return net->dtype == Y3_DTYPE_I8 && net->i8_first_conv >= 0 && slot >= net->i8_first_conv; }
inline int dtype_of_conv(const y3_net *net, int slot) { return net->dtype != Y3_DTYPE_I8 || conv_is_i8(net, slot) ? net->dtype : (int)Y3_DTYPE_F16; }
inline const ConvFamily &family_of_conv(const y3_net *net, int slot) { return *conv_family(dtype_of_conv(net, slot)); }

// What conv op `oi` launches for the rows of one call.  InStem: nothing of its own, it runs inside the Stem launch of op 1.  TinyStem: op 2 of
// a net whose ops 0..3 run as the fused tiny stem; InTinyStem: op 0 of it (the two pools between are skipped by the forward).
enum class ConvKind { First, Stem, InStem, HeadDecodeF32, Mfma, SplitK, TinyStem, InTinyStem };
struct ConvChoice {
    ConvKind kind;
    int tile;      // Mfma, SplitK: tile id of the family's table
    int k_chunk;   // ConvArgs::k_chunk
    int xcd_gn;    // ConvArgs::xcd_gn
    int split_k;   // SplitK: slices
    const uint32_t *pos_tab;   // ConvArgs::pos_tab (fp32 border skip), null: raster rows
    int border_tiles;          // ConvArgs::border_tiles (with pos_tab: the balanced tile -> XCD mapping), -1: the raster launches' mapping
};
// The one launch decision.  `a`: the slice's ConvArgs (rows of the call, byte sizes, a.dec set when the conv decodes its own tiles).
ConvChoice choose_conv(const y3_net *net, int oi, const ConvArgs &a);
ConvChoice choose_conv_planned(const y3_net *net, int oi);   // ... for max_batch images, as a plain forward launches it
int conv_op(const y3_net *net, int slot);                    // the op that runs conv `slot`, -1: none
// The first conv slot for which the planned mode (an int8 plan: fp16 before the cut, int8 from it on) has no tile that fits -- neither
// a forced one nor the chooser's -- or -1 when every conv has one.  y3_net_plan_hw, once the mode, the cut and out_slot are known.
int conv_without_tile(const y3_net *net);

bool stem_applicable(const y3_net *net);
bool stem_conv2_applicable(const y3_net *net);
void resolve_stem(y3_net *net);   // stem_fused / stem_conv2 of a planned net from the planned mode's switch and the graph
bool tiny_stem_applicable(const y3_net *net);
void resolve_tiny_stem(y3_net *net);   // tiny_stem_fused / tiny_inner from y3_net_set_tiny_stem_fusion, the planned mode and the graph (y3_net_plan, before conv_without_tile)
bool output_staged(const y3_net *net, int t);
y3_status resolve_splits(y3_net *net);
// fp32 plans: the position table of every 3x3 single-source conv's geometry, built and uploaded once per geometry (y3_net_plan)
y3_status resolve_border(y3_net *net);
// int8 plans: the cut, the element size of every tensor and the scales the plan needs (y3_net_plan, before the arena is placed) ...
y3_status resolve_i8(y3_net *net);
// ... the cut itself, from the graph alone (the conv count: no conv qualifies) ...
int i8_cut(const y3_net *net);
// ... and, with y3_net_set_pools_i8, which aux ops run in int8 behind that cut (aux_i8, null: only the check) or why the graph is refused;
// from the graph alone, so y3_net_plan asks before it frees the plan in force
y3_status resolve_i8_aux(const y3_net *net, int cut, std::vector<char> *aux_i8, std::vector<char> *behind);
// ... and the epilogue scales of int8 conv `slot` on the device, once its weights are loaded (y3_net_plan; y3_net_set_conv_weights on a planned net)
y3_status upload_i8_scales(y3_net *net, int slot);
void free_plan(y3_net *net);
// free_plan and "no plan" in every field an entry point asks: a plan refused or failed after the old one was freed leaves this
void drop_plan(y3_net *net);

// y3_net_detect scratch for `batch` images: grid sizes {gh, gw} of the net's heads, boxes per image, byte offsets of the parts and their total
struct DetectLayout {
    int32_t gs[3][2];
    size_t n_boxes;
    size_t grid[3], boxes, cls, scores, sel, nms_ws, total;
    // behind the NMS workspace (nms_bytes of it), the multi-label route's own parts: candidate sources [batch,N] i32, totals [batch] i32,
    // and the per-box counts of y3_yolo_decode_candidates_hw (cand_ws_bytes).  Its candidates lie in boxes / cls / scores (capacity <= N).
    size_t nms_bytes, cand_src, totals, cand_ws, cand_ws_bytes;
};
DetectLayout detect_layout(const y3_net *net, int batch);

// y3_yolo_decode_scores_hw_n under the caller's name `who`
y3_status decode_scores_hw(const char *who, const float *const *grids_dev, const int32_t (*grid_hw)[2], int n_scales, int batch, int nclasses,
                           const float *anchors_host, float *bboxes_dev, int64_t *class_idx_dev, float *scores_dev, void *stream);

// y3_yolo_decode_candidates_hw_n under the caller's name `who`
y3_status decode_candidates_hw(const char *who, const float *const *grids_dev, const int32_t (*grid_hw)[2], int n_scales, int batch, int nclasses,
                               const float *anchors_host, float score_threshold, int capacity, float *cand_boxes_dev, int64_t *cand_cls_dev,
                               float *cand_scores_dev, int32_t *cand_src_dev, int32_t *totals_dev, void *workspace_dev, size_t workspace_bytes,
                               void *stream);

// The detection tail, once: what follows the decode (or the candidates) in y3_net_detect[_grids] and the merge kernels in
// y3_merge_tile_detections.  select_check: the threshold rules of the NMS of `nms_mode` (Y3_NMS_*) under the caller's name -- run it before the
// call's first launch, so that a refused call enqueues nothing.  select_and_pack: the padded NMS of nms_mode over [batch, n] rows, the pack
// into `packed`, and with cand_src (multi-label; null: single label) the rewrite of the packed index words to the candidates' boxes.
y3_status select_check(const char *who, int nms_mode, float iou_threshold, float score_threshold);
y3_status select_and_pack(const char *who, const float *boxes, const float *scores, const int64_t *cls, const int32_t *cand_src, int batch, int n,
                          int max_boxes, int nms_mode, float iou_threshold, float score_threshold, int32_t *sel, int32_t *num_valid, void *ws,
                          size_t ws_bytes, void *packed, void *stream);

}  // namespace y3
