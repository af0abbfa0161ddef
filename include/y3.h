/*
 * y3.h -- C ABI of the MI355X-native YOLOv3 inference path (liby3hip.so).
 *
 * The reference (ronen-halevy/yolo-v3-tf2) has no FFI of its own: its operator surface is
 * three Python callables and one Keras Layer that hand tensors to the TensorFlow runtime.
 * This header declares the entry points a binding for that surface calls instead; each one
 * cites the reference interface it replaces.  The ctypes binding the package itself uses is
 * yolo-v3-tf2_amd/_lib.py; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - plain C types only; every function returns y3_status (0 = OK, <0 = error) and never
 *     throws or aborts: each entry point that can reach a host allocation is a function-try-block, so a failed allocation
 *     comes back as Y3_ERR_OOM (any other C++ exception as Y3_ERR_INTERNAL) with a message, not as a terminated host process.
 *     y3_last_error() returns a thread-local message for the last failure (a fixed buffer: reporting allocates nothing).
 *   - "dev" pointers are device (HBM) addresses owned by the caller (e.g. torch `data_ptr()`);
 *     "host" pointers are ordinary host memory, copied during the call.
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing
 *     synchronises the device unless stated.  A y3_net is bound to the device that was current
 *     at creation and is not thread-safe.  Calls on a net (plan, weights, forward, detect, measure) run on the
 *     net's device whatever the caller's current device is and leave the caller's current device as they found it.
 *   - tensors are NHWC fp32 unless stated; boxes are normalised (xmin,ymin,xmax,ymax).
 */
#ifndef Y3_H
#define Y3_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int y3_status;
enum {
    Y3_OK = 0,
    Y3_ERR_INVALID = -1,   /* bad argument / unsupported shape */
    Y3_ERR_HIP = -2,       /* HIP runtime error */
    Y3_ERR_OOM = -3,       /* device allocation failed */
    Y3_ERR_STATE = -4,     /* call order (weights missing, plan missing, ...) */
    Y3_ERR_NODEVICE = -5,  /* no usable GPU */
    Y3_ERR_COMM = -6,      /* RCCL error (or librccl not loadable) */
    Y3_ERR_INTERNAL = -7   /* a C++ exception other than std::bad_alloc (reported as Y3_ERR_OOM) was stopped at the boundary */
};

/* activation storage / MFMA input type of the conv stack */
enum { Y3_DTYPE_F32 = 0, Y3_DTYPE_BF16 = 1, Y3_DTYPE_F32X3 = 2, Y3_DTYPE_F32X2 = 3, Y3_DTYPE_F16 = 4, Y3_DTYPE_I8 = 5 };

int y3_version(void);
const char *y3_last_error(void);
/* number of visible HIP devices (0 when none); never fails */
int y3_device_count(void);
/* 1 when tile id `tile` of the conv kernel family of `dtype` (Y3_DTYPE_*) exists in this library, else 0.  Tile ids are stable
 * (tuning tables refer to them); the ids of tiles that were measured and lost in rounds 1-4 (timing-only ablations, the
 * stream-K schedule, residual prefetch, the pipelined bf16 tile, bf16 tap-row reuse and the four-wave 256x256 bf16 tile;
 * DESIGN.md section 4, records under profiles/) are retired and answer 0.  Every id that answers 1 is named by a packaged
 * tuning table or chosen by the library's heuristic for some conv (tests/test_abi.py).  Y3_DTYPE_F16 shares the bf16 family's tile
 * table: it answers what Y3_DTYPE_BF16 answers. */
int y3_tile_built(int dtype, int tile);

/* ------------------------------------------------------------------------------------------
 * Network = the fused conv program.
 * Replaces: the Keras Model built by ParseModel.build_model (reference: core/parse_model.py:279-314)
 * and executed by model(inputs) / model.predict (reference: inference.py:109,125,161).
 * One y3_conv_desc is one launch: Conv2D [+BatchNormalization] [+LeakyReLU(0.1)] [+Add] with the
 * optional UpSampling2D(2)+Concatenate feeding a 1x1 conv read in place
 * (reference: core/parse_model.py:13-56,59-75,102-160).
 * ---------------------------------------------------------------------------------------- */
typedef struct y3_net y3_net;

typedef struct {
    int32_t size;          /* kernel size: 1 or 3 */
    int32_t stride;        /* 1, or 2 (3x3 only: top/left zero pad then 'valid') */
    int32_t cin;           /* total input channels */
    int32_t cout;
    int32_t bn;            /* 1: BatchNormalization(eps) after the conv, no bias; 0: bias */
    int32_t leaky;         /* 1: LeakyReLU(alpha=0.1) */
    int32_t src0;          /* tensor id of input channels [0, c0) */
    int32_t src0_upsample; /* 1: src0 is half resolution and read through nearest x2 up-sampling */
    int32_t c0;            /* channels taken from src0 (== cin when src1 < 0) */
    int32_t src1;          /* -1, or tensor id of input channels [c0, cin) */
    int32_t residual;      /* -1, or tensor id added after the activation (shortcut) */
    int32_t dst;           /* tensor id written */
    int32_t in_div;        /* input spatial size  = image_size / in_div  (after up-sampling) */
    int32_t out_div;       /* output spatial size = image_size / out_div */
} y3_conv_desc;

/* auxiliary ops that the lowering could not fold into a conv (not used by YOLOv3 itself), and the two max-pools of YOLOv3-tiny, which are
 * never folded: MaxPooling2D(2, strides 2 | 1, 'same') of src0 into dst (y3_maxpool2x2 below states the rule), src1 = -1.  Add, up-sample
 * and concat run in Y3_DTYPE_F32 plans only; the pools run in Y3_DTYPE_F32, _BF16 and _F16 plans on the plan's stored elements, and
 * y3_net_plan refuses a net that holds one in Y3_DTYPE_F32X3, _F32X2 and _I8 (plane-split tensors and calibrated pools are not built). */
enum { Y3_AUX_ADD = 0, Y3_AUX_UPSAMPLE2X = 1, Y3_AUX_CONCAT = 2, Y3_AUX_MAXPOOL2X2_S2 = 3, Y3_AUX_MAXPOOL2X2_S1 = 4 };
typedef struct {
    int32_t kind;
    int32_t src0;
    int32_t src1; /* -1 for upsample */
    int32_t dst;
} y3_aux_desc;

typedef struct {
    int32_t channels;
    int32_t div; /* spatial size = image_size / div */
} y3_tensor_desc;

/* op_kinds[i] == 0: take the next y3_conv_desc; == 1: take the next y3_aux_desc (execution order).
 * tensors[0..n_tensors) describes every tensor id; `input_tensor` is the image, `outputs[3]` the head
 * outputs in model order (coarsest grid first), each with 3*(5+nclasses) channels.
 * Conv widths.  Accepted here: Cin a multiple of 32 (3 for the first layer), any Cout; a two-source conv (1x1 only) with c0 and
 * cin - c0 multiples of 32.  What a mode then runs is decided by its tile tables, and y3_net_plan refuses a mode in which some conv
 * has no tile (Y3_ERR_INVALID, naming the conv, its Cin / c0 / Cout and the mode) before it allocates anything:
 *   Y3_DTYPE_F32, _F32X3, _F32X2: every accepted conv (K tiles of 32 channels; Cout padded to 32, the plane-split modes to 64).
 *   Y3_DTYPE_BF16, _F16: K tiles of 64 channels where Cin and the concat boundary c0 are multiples of 64, any Cout; else the K tiles
 *     of 32 channels, which exist 64 wide only: Cout rounded up to 32 must then be a multiple of 64 (Cin = 96 -> Cout = 192 runs,
 *     96 -> 96 and 32 -> 32 are refused; so is [96, 96] -> 96).
 *   Y3_DTYPE_I8: the convs before the cut as _F16; from the cut on Cin and c0 are multiples of 128 by the cut's own rule, any Cout. */
y3_status y3_net_create(const y3_tensor_desc *tensors, int n_tensors, const int32_t *op_kinds, int n_ops,
                        const y3_conv_desc *convs, int n_convs, const y3_aux_desc *aux, int n_aux,
                        int input_tensor, const int32_t outputs[3], int nclasses, y3_net **out);
/* The same for a net of n_outputs heads, 2 (YOLOv3-tiny: 1/32 and 1/16) or 3: outputs[n_outputs].  y3_net_create IS this call with 3.
 * y3_net_heads reports the count (0 for a null net).  Every net-level call that takes or fills per-head arrays -- y3_net_forward,
 * y3_net_forward_decode, y3_net_detect, y3_net_detect_grids, y3_net_profile_convs, the measure_sclk calls -- reads the first
 * y3_net_heads entries of its pointer arrays and never the rest; anchors_host is [heads][3][2]; N per image is 3 * sum over the heads
 * of gh * gw (2535 at 416 x 416 with two heads).  NMS, pack, the evaluation counters, AP matching, the tile merge and un-letterbox
 * work on boxes and packed rows and know nothing of heads.  y3_yolo_assign_targets / y3_yolo_loss stay three-scale.
 * A pool op (Y3_AUX_MAXPOOL2X2_*) needs a source of a channel count that is a multiple of 32 in every mode that runs it. */
y3_status y3_net_create_heads(const y3_tensor_desc *tensors, int n_tensors, const int32_t *op_kinds, int n_ops,
                              const y3_conv_desc *convs, int n_convs, const y3_aux_desc *aux, int n_aux,
                              int input_tensor, const int32_t *outputs, int n_outputs, int nclasses, y3_net **out);
int y3_net_heads(const y3_net *net);
void y3_net_destroy(y3_net *net);

/* Weights of conv `conv_slot` (index into the `convs` array given at creation), host pointers.
 * w is HWIO [size,size,cin,cout] (the Keras Conv2D kernel layout, reference: convert.py:61-68).
 * bn convs: gamma/beta/mean/var [cout], eps (Keras default 1e-3); bias convs: bias [cout], others NULL.
 * Replaces model.load_weights(...) (reference: inference.py:102). */
y3_status y3_net_set_conv_weights(y3_net *net, int conv_slot, const float *w, const float *gamma,
                                  const float *beta, const float *mean, const float *var, const float *bias,
                                  float eps);

/* Setters on a planned net.  A y3_net lives long and is planned again and again (another batch, canvas or mode); every y3_net_set_* and
 * y3_net_keep_activations may be called before the first plan, between plans and on a planned net, and states below which of two things
 * it does on a planned net:
 *   ACTS AT ONCE -- the very next forward / detect runs as a fresh net would that was configured that way before its one plan:
 *     y3_net_set_lanes, y3_net_set_tile / _bf16 / _x3 / _x2, y3_net_set_low_latency* and y3_net_set_split_k*, y3_net_set_stem_fusion /
 *     _f16, y3_net_set_k_chunk, y3_net_set_border_skip, y3_net_set_xcd_mode, y3_net_set_nms_mode, y3_net_set_multi_label.
 *   WAITS FOR THE NEXT PLAN -- the planned net keeps running, bit for bit, what it ran before the call; y3_net_plan reads the value:
 *     y3_net_set_tiny_stem_fusion, y3_net_set_pools_i8, y3_net_set_early_chunk, y3_net_keep_activations, y3_net_set_act_scales (they
 *     decide the arena).
 *     The plan keeps its own copy of what it read; no decision of a planned net reads the live value.
 * Every setting survives y3_net_plan: a plan changes none of them.  y3_net_set_conv_weights on a planned net acts at once, in every
 * format, the int8 epilogue scales of the plan in force included.  (tests/test_lifecycle_gpu.py holds a long-lived net to this.)
 * Tuning/testing knobs (no reference counterpart).
 * y3_net_set_tile: force the block tile of one conv (index into the kernel's tile table; -1 = heuristic).
 * A tile that cannot serve the conv (shape, or a bf16-only tile on a conv that writes an fp32 net output) is refused here with
 * Y3_ERR_INVALID and a message, not by the forward.
 * On a planned net the forced tile acts at once (the split decision of the plan is made again with it); it survives y3_net_plan.
 * y3_net_keep_activations(1) before y3_net_plan: no buffer reuse, so y3_net_read_tensor can read any
 * intermediate after a forward.  On a planned net it waits for the next plan: the arena, the fused stem (which needs buffer reuse) and
 * the route y3_net_detect takes stay those of the plan in force.
 * y3_net_set_tile_bf16 acts on both 16-bit plans: Y3_DTYPE_BF16 and Y3_DTYPE_F16 plans share the tile ids, the heuristic and this
 * per-conv forced tile (no fp16 table is tuned or shipped). */
y3_status y3_net_set_tile(y3_net *net, int conv_slot, int tile);
y3_status y3_net_set_tile_bf16(y3_net *net, int conv_slot, int tile);
y3_status y3_net_set_tile_x3(y3_net *net, int conv_slot, int tile);
y3_status y3_net_set_tile_x2(y3_net *net, int conv_slot, int tile);   /* same tile table as _x3; a subset is built */
/* y3_choose_tile (pure, no device): the tile id the heuristic of plan mode `dtype` (Y3_DTYPE_*; Y3_DTYPE_I8: the int8 family) gives a
 * conv of this shape -- no forced tile, no tuning table -- through the functions the launch decision itself calls.  c0: channels of
 * the first source of a two-source 1x1 conv, -1 for one source.  M: GEMM rows (images x output positions) of the call, M_plan: of the
 * planned batch.  arena_out: 1 when the launch stores the mode's own format, 0 when it writes an fp32 net output itself.  Returns -1
 * when no built tile of the mode fits the conv (y3_net_plan refuses such a net in that mode), -2 for a shape y3_net_create refuses
 * or an unknown dtype. */
int y3_choose_tile(int dtype, int size, int stride, int cin, int c0, int cout, long long M, long long M_plan, int arena_out);
/* Run a forward as `lanes` (1..4) equal sub-batches: the first on the caller's stream itself, the others on forked
 * internal streams joined back into it: the tail of one sub-batch's conv kernel overlaps the next kernel of another.
 * Results are unchanged (images are independent).  Falls back to fewer lanes when the batch is not divisible.
 * Acts at once on a planned net (the split-K workspace grows to one region per lane). */
y3_status y3_net_set_lanes(y3_net *net, int lanes);
/* Placement of the fp32 conv tiles on the 8 XCDs (each has a private 4 MB L2).  1 (default): per conv, the XCDs form an
 * (8/gn) x gn grid over the (pixel-tile, channel-tile) matrix, gn chosen so that an XCD's slice of the weights stays in
 * its L2 (the 256->512 / 512->1024 3x3 weights are 4.7 / 18.9 MB); 0: every XCD takes a contiguous run of tiles.
 * Results are bit-identical in both modes (same per-tile arithmetic).  A batch-minor launch (border skip, below) splits its border
 * tiles, whose K walks are short, and its interior tiles evenly over the XCD pixel-tile ranges of either mode (8 ranges in mode 0).
 * Read by every forward: acts at once on a planned net. */
y3_status y3_net_set_xcd_mode(y3_net *net, int mode);
/* K order of the fp32 3x3 convs.  channels > 0 (a multiple of 32): for every chunk of that many input channels all 9 taps,
 * then the next chunk, so that the 9 reads of a pixel (one per tap) fall close together in time and hit in L2 (the tap-
 * major order re-fetched the operands of the 13x13 layers ~18x from beyond L2).  The same products in another summation
 * order: results differ from the tap-major ones in the last bits.  0: tap-major; -1 (default): chosen per conv.
 * Read by every forward: acts at once on a planned net. */
y3_status y3_net_set_k_chunk(y3_net *net, int channels);
/* Border skip of the fp32 3x3 convs.  A 3x3 conv with pad 1 multiplies zeros wherever a tap of a border pixel falls outside the image
 * (10 % of the products at 13^2).  Where a call's images come in whole blocks of 32 (batch % 32 == 0 per lane), an fp32 plan runs its
 * single-source 3x3 convs (not the first layer, the fused stem, the weight-resident tile 33 or a split-K conv) with GEMM rows ordered
 * position-major, batch-minor over a table of output positions sorted by which taps read inside the image, and every workgroup leaves
 * out the taps that are padding for all of its positions.  Only products with zero are left out: results are bit-identical for finite
 * weights (a non-finite weight met 0 * inf = NaN at the border before and is skipped now).  mode -1 (default): the library's rule,
 * 0: off, 1: on wherever legal.  Read by every forward (acts at once on a planned net); other plans and ineligible convs launch what they always did.
 * y3_net_get_border_skip: in how many of its sub-batches (y3_net_set_lanes) a forward of `batch` images launches conv `conv_slot` of the
 * planned net that way under the mode in force (0: the raster launch everywhere, or no plan).
 * y3_border_order (pure, no device): the position table of one conv geometry, Ho * Wo entries ho << 20 | wo << 9 | mask9, bit u * 3 + v of
 * mask9 = input pixel (ho * stride - pad + u, wo * stride - pad + v) lies inside H x W; stably sorted by
 * (number of bits set in mask9, mask9): positions of one mask stay together, in raster order.  Ho, Wo <= 2047.
 * y3_border_tile_map (pure, no device): the workgroup -> tile mapping of such a launch, from the function its kernel evaluates.  T pixel
 * tiles, the first Tb of them border tiles, gm in {1, 2, 4, 8} XCD pixel-tile ranges of 8 / gm XCDs each, tilesN channel tiles (a multiple
 * of 8 / gm).  Returns the launch's grid size, -1 for arguments no launch has; out, unless null, receives (pixel tile, channel tile) per
 * workgroup, (-1, -1) for a padding workgroup that exits at once.  Workgroup b runs on XCD b % 8, range (b % 8) / (8 / gm); every range
 * holds its share of border tiles [x Tb / gm, (x + 1) Tb / gm) and of interior tiles. */
y3_status y3_net_set_border_skip(y3_net *net, int mode);
int y3_net_get_border_skip(const y3_net *net, int conv_slot, int batch);
void y3_border_order(int Ho, int Wo, int H, int W, int stride, int pad, uint32_t *out);
int y3_border_tile_map(int T, int Tb, int gm, int tilesN, int32_t *out);
/* Low-latency fp32 plans: split-K convs for small batches (one to eight images), off by default.
 * At one 416^2 image the convs of the 13^2 .. 52^2 grids launch 24 .. 172 workgroups on 256 compute units, each walking the whole
 * K = taps * Cin alone.  With y3_net_set_low_latency(net, 1), called before y3_net_plan, each eligible conv is cut along K into S slices
 * that run as S times the workgroups; every slice stores its raw accumulators into a workspace owned by the plan, and a second launch on
 * the same stream adds the slices in the fixed order 0, 1, ..., S-1 and applies the epilogue (no atomics: two runs give the same bits).
 * S is decided at plan time by y3_choose_split_k from the conv's shape, its tile at the planned max_batch and the device's compute
 * units -- never from the rows of a call, so inside one plan an image's result does not depend on its batch or position.  S = 1 (the
 * ordinary launch) wherever the planned batch already fills the chip.  Never split: the first layer, the fused stem, the weight-
 * resident tile 33, the three detection-head convs (y3_net_detect and the composed route stay bit-identical), and -- by these three calls --
 * any plan that is not Y3_DTYPE_F32 (a Y3_DTYPE_BF16 plan splits through the _bf16 calls below, a Y3_DTYPE_F16 plan through the _f16
 * calls; the plane-split modes never split).
 * The same products in another summation order: results differ from the default plan's in the last bits (as
 * y3_net_set_k_chunk says of itself).  With it off nothing changes.
 * y3_net_set_split_k: S of one conv: -1 = y3_choose_split_k when low latency is on (else 1), 1 = off, 2..16 = that value whether or not
 * low latency is on.  An ineligible conv or S > the conv's K tiles (K / 32) is refused here with Y3_ERR_INVALID and a message, not
 * by the forward.  y3_net_get_split_k: the value in force after planning (1 before).
 * y3_choose_split_k (pure, no device): 1 when tiles >= 2 * n_cus; else the smallest S with tiles * S >= 2 * n_cus, capped at
 * k_tiles / 4, at 16 and at 16 MiB of slabs (S * slab_bytes_per_slice); tiles = workgroups of the unsplit launch.
 * On a planned net the switch and the request act at once, here and in the _bf16 / _f16 / _i8 calls below: the decision of the plan in
 * force is made again from the same plan-time quantities and the workspace grows if it must.  Switches and requests of every mode
 * survive y3_net_plan, also a plan in another mode, where they rest. */
y3_status y3_net_set_low_latency(y3_net *net, int on);
y3_status y3_net_set_split_k(y3_net *net, int conv_slot, int S);
int y3_net_get_split_k(const y3_net *net, int conv_slot);
int y3_choose_split_k(long long tiles, int k_tiles, int n_cus, long long slab_bytes_per_slice);
/* Low-latency bf16 plans: the same for Y3_DTYPE_BF16 plans, with a switch, a request and a decision of their own beside the fp32 ones
 * (the fp32 calls above keep answering for fp32 plans only: y3_net_get_split_k is 1 on a bf16 plan, y3_net_set_split_k refuses one).
 * The rule and its inputs are the same -- y3_choose_split_k on the conv's shape, its bf16 tile at the planned max_batch and the compute
 * units -- with K tiles of 64 (K / 64), and only for convs of at least 32 K tiles (K >= 2048: measured, the shorter launches lose to the
 * second launch; a forced S is taken as given).  A slice stores raw fp32 accumulators; the second launch adds the slices in the order 0, 1, ...,
 * S-1 and applies the unsplit epilogue's own operations (* scale + shift, leaky, + the bf16 shortcut, one rounding to bf16), so equal
 * sums give the unsplit launch's bits.  Never split in a bf16 plan: the first layer and the convs inside the fused stem, the weight-
 * resident tile 32, the BK = 32 tiles (Cin = 32 layers), any conv whose tile at the planned rows is not 11 or 12 (the 64x64 and 64x128
 * LDS-DMA tiles: the only ones with a split form), a conv storing bf16 with Cout % 8 != 0, the three detection-head convs.
 * y3_net_set_low_latency_bf16: 0 / 1, off by default.  y3_net_set_split_k_bf16: -1 = the rule when the bf16 switch is on (else 1), 1 = off,
 * 2..16 forced; an ineligible conv, S > K / 64, or a forced value on a planned net whose dtype is not Y3_DTYPE_BF16 is refused with
 * Y3_ERR_INVALID and a message.  y3_net_get_split_k_bf16: the value in force after planning; 1 before, 1 on a plan that is not bf16.
 * These three do not act on Y3_DTYPE_F16 plans: the switch splits nothing there, and a forced value on a planned fp16 net is refused like
 * on any other plan that is not bf16 ("only Y3_DTYPE_BF16 plans take a bf16 split"). */
y3_status y3_net_set_low_latency_bf16(y3_net *net, int on);
y3_status y3_net_set_split_k_bf16(y3_net *net, int conv_slot, int S);
int y3_net_get_split_k_bf16(const y3_net *net, int conv_slot);
/* Low-latency fp16 plans: the same once more for Y3_DTYPE_F16 plans, again with a switch, a request and a decision of their own (off and
 * -1 by default: an fp16 plan on which these are never called launches what it always did).  Every rule of the _bf16 three holds with
 * "fp16" for "bf16": the same kernels on the f16 MFMA, tiles 11 and 12, K tiles of 64, the floor of 32 K tiles, the finish launch adding
 * the fp32 slabs in the order 0, 1, ..., S-1 and applying the unsplit fp16 epilogue (one rounding to nearest even, IEEE overflow), so equal
 * sums give the unsplit launch's bits; the same convs are never split (the fused stem's are those of y3_net_set_stem_fusion_f16).  A forced
 * value on a planned net that is not Y3_DTYPE_F16 is refused ("only Y3_DTYPE_F16 plans take an fp16 split").  y3_net_get_split_k_f16: the
 * value in force after planning; 1 before, 1 on a plan that is not fp16 (the fp32 and bf16 getters answer 1 on an fp16 plan). */
y3_status y3_net_set_low_latency_f16(y3_net *net, int on);
y3_status y3_net_set_split_k_f16(y3_net *net, int conv_slot, int S);
int y3_net_get_split_k_f16(const y3_net *net, int conv_slot);
/* Low-latency int8 plans: the same for Y3_DTYPE_I8 plans (see "int8 plans" below), with a switch, a request and a decision of their own
 * (off and -1 by default: an int8 plan on which these are never called launches what it always did).  They act on the int8 convs, those
 * from y3_net_i8_first_conv on; the convs before the cut launch what an fp16 plan launches and stay unsplit under every switch, the
 * fp16 one included (splitting them is not built).  Tiles 11 and 12 on v_mfma_i32_32x32x32_i8, K tiles of 128 (K / 128); the rule is
 * y3_choose_split_k on the conv's shape, its int8 tile at the planned max_batch and the compute units, and only for convs of at
 * least 36 K tiles (K >= 4608: measured, profiles/latency_i8_splitk_sweep.txt -- int8 launches are short, and every shorter conv loses
 * to the second launch at some batch from 1 to 8; a forced S is taken as given).  A slice stores its
 * raw i32 accumulators (no conversion: a partial sum beyond 2^24 has no float); the second launch adds the S values as integers and
 * applies the unsplit int8 epilogue's own operations.  Integer sums do not depend on order, so a split int8 conv gives the unsplit conv's
 * bits -- and those of yolo_v3_tf2_amd/quant.py -- on all data and at every S: the low-latency int8 plan's results ARE the default int8
 * plan's.  Never split in an int8 plan: every conv before the cut (so the first layer and the stem convs), any conv whose tile at the
 * planned rows is not 11 or 12 (the 16x16x64 tiles and the 16-wave tiles have no split form), a conv storing int8 with Cout % 16 != 0,
 * the three detection-head convs.
 * y3_net_set_low_latency_i8: 0 / 1, off by default.  y3_net_set_split_k_i8: -1 = the rule when the int8 switch is on (else 1), 1 = off,
 * 2..16 forced; an ineligible conv, S > K / 128, a forced value on a planned net whose dtype is not Y3_DTYPE_I8 ("only Y3_DTYPE_I8
 * plans take an int8 split") or on a conv before the cut of a planned int8 net ("runs in fp16 in this plan") is refused with
 * Y3_ERR_INVALID and a message.  y3_net_get_split_k_i8: the value in force after planning; 1 before, 1 on a plan that is not int8 (the
 * fp32, bf16 and fp16 getters answer 1 on an int8 plan, and their setters refuse one). */
y3_status y3_net_set_low_latency_i8(y3_net *net, int on);
y3_status y3_net_set_split_k_i8(y3_net *net, int conv_slot, int S);
int y3_net_get_split_k_i8(const y3_net *net, int conv_slot);
/* The persistent kernels: a fixed grid of workgroups, each walking its tiles with tile += grid (the fused stems) or, per output-channel
 * slice, spatial tile += grid / slices (the weight-resident 3x3 convs).  Y3_PERSISTENT_*: which one.  TINY_STEM -- the fused YOLOv3-tiny
 * stem in every format, tiles of 4 x 8 pool-1 pixels, min(n_tiles, 4 * n_cus); STEM_F32 / STEM_16 -- the fused YOLOv3 stem, tiles of
 * 8 x 16 conv1 pixels, min(n_tiles, n_cus) in fp32 and min(n_tiles, 2 * n_cus) in bf16 / fp16; RES_F32 (tile id 33, tiles of 8 x 16
 * pixels) / RES_16 (16-bit tile id 32, tiles of 4 x 32 pixels) -- min(n_tiles, max(1, n_cus / slices)) * slices with slices = Cout / 64.
 * A workgroup's walk is n_tiles / (grid / slices) tiles long, one more for the first n_tiles % (grid / slices) of a slice. */
enum { Y3_PERSISTENT_TINY_STEM = 0, Y3_PERSISTENT_STEM_F32 = 1, Y3_PERSISTENT_STEM_16 = 2, Y3_PERSISTENT_RES_F32 = 3, Y3_PERSISTENT_RES_16 = 4 };
/* Workgroups the persistent kernel `kind` launches for n_tiles spatial tiles, `slices` output-channel slices (weight-resident convs;
 * 1 otherwise) on a device of n_cus compute units; <= 0: bad arguments.  Pure, no device. */
int y3_persistent_grid(int kind, long long n_tiles, int slices, int n_cus);
/* Lane regions.  A forward of `batch` images on `lanes` concurrent sub-batches (y3_net_set_lanes; a forward uses min(lanes, batch))
 * gives lane l the images [start[l], start[l+1]), start[l] = batch * l / lanes, and every arena block of block_bytes bytes is cut into one
 * region per lane.  y3_lane_offset is the byte offset of lane `lane`'s region from the block start -- the function every launch's
 * addresses come from:
 *     off[0] = 0,   off[l] = roundup256(off[l-1] + ceil(block_bytes * (start[l] - start[l-1]) / batch))
 * Every offset is a multiple of 256; a region holds its lane's share of the block, ceil(block_bytes * nb / batch) >= nb * image bytes of
 * any tensor that fits the block at `batch` images, before the next one starts, so two lanes never share a byte; the last region ends
 * fewer than 256 * lanes bytes past the block, inside the 4096 bytes of slack every block is allocated with.  Where
 * block_bytes * start[l] / batch is a multiple of 256 for every lane the regions are contiguous: off[l] is that value.
 * -1: block_bytes < 0, batch < 1, lanes outside 1..4 or above batch, lane outside [0, lanes).  Pure, no device. */
long long y3_lane_offset(long long block_bytes, int batch, int lanes, int lane);
y3_status y3_net_keep_activations(y3_net *net, int keep);
/* 1 (default): when the program starts with conv0 (3x3/1, 3 -> 32) feeding only conv1 (3x3/2, 32 -> 64) -- the Darknet-53
 * stem, reference config/models/yolov3/backbone.yaml layers 1-2 -- and the plan is fp32 or bf16 without keep_activations,
 * (this call does not act on Y3_DTYPE_F16 plans: one launch per conv whatever it is set to, unless y3_net_set_stem_fusion_f16 below),
 * the two run as ONE kernel that keeps conv0's output (the largest tensor of the network, 1.4 GB at 64 x 416^2) in LDS; the
 * 1x1 conv that follows (64 -> 32, backbone.yaml layer 3) is computed by the same kernel from conv1's tile.
 * 2: conv0 + conv1 in one kernel, the 1x1 conv as its own launch (bf16 plans: bit-identical to 1).
 * 0: one launch per conv.  fp32 plans: results agree to fp32 rounding (conv0's summation order differs between the two
 * kernels).  bf16 plans: the fused kernel forms conv0's products on the bf16 matrix cores from operands split x = hi + lo
 * (hi*hi + hi*lo + lo*hi, fp32 accumulation: ~2^-16 relative error per product, NOT fp32 arithmetic) and rounds the result to
 * bf16 where the pipeline stores it; against the one-launch-per-conv form a fraction of a percent of conv0's bf16 values round
 * the other way (bounded by tests/test_gpu_parity.py::test_fused_stem_bf16_matches_oracle_and_the_two_launch_form).
 * Acts at once on a planned net of a mode it acts on (the split decision is made again: a conv inside the fused stem is not split);
 * "without keep_activations" is what the plan in force was made with. */
y3_status y3_net_set_stem_fusion(y3_net *net, int on);
/* The same switch for Y3_DTYPE_F16 plans, and for them only: 0 (default: one launch per conv, as an fp16 plan always ran), 1, 2 with the
 * meanings above; it does not act on a plan of any other mode, as y3_net_set_stem_fusion does not act on an fp16 plan.  The graph decides
 * as for bf16.  The kernel is the bf16 one on v_mfma_f32_32x32x16_f16, every rounding the fp16 round-to-nearest-even of the fp16 convs
 * (2: bit-identical to 1).  conv0's products come from operands split v = hi + lo' * 2^-11 with hi = |v| < 2^-14 ? 0 : fp16(v) and
 * lo' = fp16((v - hi) * 2048): per K step of 16 the cross terms lo'_x hi_w + hi_x lo'_w are summed on their own, that sum times 2^-11 is the
 * C input of the hi_x hi_w terms (~2^-22 relative error per product; lo' lo' dropped).  conv0's weights are divided per output channel by
 * the power of two that brings the channel's largest magnitude into [1, 2), and the channel's scale multiplied by it, both exactly, so
 * the accuracy does not depend on the weights' magnitude and no operand that matters is subnormal (nothing relies on what the matrix
 * pipe does with one).  Against the one-launch-per-conv fp16 plan a fraction of a percent of conv0's fp16 values round the other way
 * (bounded by tests/test_f16_stem_gpu.py).  Precondition: pixel values finite and of magnitude at most 65504 -- a larger one makes hi
 * infinite and the result NaN, where the unfused fp16 plan only overflows at its outputs.  Acts at once on a planned fp16 or int8 net. */
y3_status y3_net_set_stem_fusion_f16(y3_net *net, int on);
/* The fused stem of YOLOv3-tiny (csrc/conv_tiny_stem.hip), a switch of its own: 0 (default) one launch per op; 1: when the program starts
 * with conv0 (the 3x3/1 first layer, 3 -> 16 stored as 32) -> Y3_AUX_MAXPOOL2X2_S2 -> conv1 (3x3/1, 16 stored as 32 -> 32, single source,
 * no shortcut) -> Y3_AUX_MAXPOOL2X2_S2, each of the first three outputs has exactly one reader, none of the four is a net output and there
 * are no early chunks, a Y3_DTYPE_F32, Y3_DTYPE_BF16 or Y3_DTYPE_F16 plan runs the four as ONE launch at the real widths 16 and K = 144:
 * conv0's tensor, pool 0's and conv1's never reach memory, and the 32 -> 32 conv, for which the 16-bit modes have no tile, never asks for
 * one -- so such a net plans in the 16-bit modes, which refuse it with the switch off.  Where the rule does not hold the switch is ignored.
 * Read by y3_net_plan: set it before planning; on a planned net it waits for the next plan (the arena of the plan in force has, or has
 * not, the three tensors).  y3_net_set_stem_fusion / _f16 do not act on it, and it does not act on them; anything but
 * 0 or 1 is Y3_ERR_INVALID.  Arithmetic: conv0 in fp32 from fp32 weights in every mode, in the stand-alone first-layer launch's order
 * (acc * scale + shift, leaky, one rounding to the plan's format); conv1 on v_mfma_f32_32x32x2_f32 (fp32 plans) or v_mfma_f32_32x32x16_bf16
 * / _f16 from 16-bit weights and the 16-bit pooled patch, fp32 accumulation, one rounding before pool 1; both pools compare values and keep
 * the winner's bits (y3_maxpool2x2's order).  conv0's stored channels 16..31 must be the lowering's zero pad channels (scale 0, shift 0):
 * a forward on other weights is refused with Y3_ERR_INVALID.  y3_net_keep_activations does not switch the fusion off: the three tensors
 * inside the launch are not stored, and y3_net_read_tensor on one of them is refused with Y3_ERR_STATE and a message naming this switch.
 * The convs inside are never split (a forced split-K on one is refused by name).
 * y3_net_get_tiny_stem_fused: 1 when the planned net runs the fused launch, 0 otherwise, also before a plan. */
y3_status y3_net_set_tiny_stem_fusion(y3_net *net, int on);
int y3_net_get_tiny_stem_fused(const y3_net *net);
/* Measurement aid (bench.py): the shader clock the chip holds under this network's load.  Runs `forwards` forwards back to
 * back (grids_dev as for y3_net_forward); in the last one, thread 0 of the middle workgroup of the conv with the most FLOPs (fp32
 * plans: an MFMA conv launch; bf16 plans, and fp16 plans with y3_net_set_stem_fusion_f16: the fused stem kernel) reads s_memtime and s_memrealtime at its entry and after
 * its epilogue: MHz = d(memtime) / d(memrealtime) x 100 (MI355X_MICROARCH.md, DVFS give-back item 6).  Synchronises the
 * stream.  No product launch carries stamps (the kernels test a null pointer).  The three measure_sclk calls temporarily
 * change the net's lane count and stamp fields: never run them concurrently with a forward on the same net. */
y3_status y3_net_measure_sclk(y3_net *net, const float *images_dev, int batch, float *const grids_dev[3], int forwards,
                              float *mhz_out, void *stream);
/* The same measurement on the launch of conv slot `conv` (tools/sclk_per_layer.py: the clock differs from layer to layer
 * with the power each one draws).  Y3_ERR_STATE when that conv's kernel carries no stamps in this plan. */
y3_status y3_net_measure_sclk_conv(y3_net *net, const float *images_dev, int batch, float *const grids_dev[3], int forwards,
                                   int conv, float *mhz_out, void *stream);
/* ... and on every conv launch of ONE forward (the last of `forwards`): mhz_out[n_convs] (0 where the conv's kernel
 * carries no stamps or runs inside another launch), and -- when not NULL -- start_us / end_us [n_convs]: when the
 * first workgroup of each launch began and when its clock-stamped (middle) workgroup ended on the chip's 100 MHz
 * real-time counter, relative to the earliest stamp: the timeline of the conv stack with no host event in it; the
 * difference of consecutive starts is a launch's duration in the real forward (bench.py: time-weighted clock). */
y3_status y3_net_measure_sclk_all(y3_net *net, const float *images_dev, int batch, float *const grids_dev[3], int forwards,
                                  float *mhz_out, double *start_us, double *end_us, void *stream);
/* Before y3_net_plan: run the first n_convs convs chunk_images images at a time, then the rest of the network on the
 * whole batch.  The first layers' activations are the largest tensors of the network (1.4 GB for 64 images at 416x416);
 * in chunks they are still in the Infinity Cache when the next conv reads them.  Results are unchanged (images are
 * independent).  0, 0 switches it off.  On a planned net it waits for the next plan: the plan keeps the segment and the chunk size it
 * was made with (the chunked tensors have blocks of their own), and a forward steps through a chunked segment by that size, at least 1. */
y3_status y3_net_set_early_chunk(y3_net *net, int n_convs, int chunk_images);
/* How many leading ops the plan in force runs in chunks (0: none, or no plan) and, through *chunk_images unless null, of how many
 * images: what the plan was made with, whatever the setter was called with since. */
int y3_net_get_early_chunk(const y3_net *net, int *chunk_images);

/* Allocate the activation arena for batches up to `max_batch` of image_size x image_size inputs
 * and select the conv arithmetic type (Y3_DTYPE_*).  May be called again to re-plan.
 * Y3_DTYPE_BF16: intermediate activations and weights are bf16 (v_mfma_f32_32x32x16_bf16, fp32 accumulate and
 * epilogue); the image batch stays fp32 (the Cin = 3 first layer reads it directly) and the head grids stay fp32.
 * Y3_DTYPE_F32X3: fp32-accurate arithmetic on the bf16 matrix cores -- every value is held as three bf16 planes
 * (x = hi + mid + lo exactly) and each product uses its six leading partial products with fp32 accumulation; same
 * image / head-grid conventions, same parity bar as Y3_DTYPE_F32.
 * Y3_DTYPE_F32X2: the same idea on the fp16 matrix cores with two planes per value, x = h + l' * 2^-11
 * (h = fp16(x), l' = fp16((x - h) * 2^11)), three partial products per product (h*h, h*l', l'*h) in two fp32
 * accumulators: representation error 2^-22 |x| (fp32: 2^-24), half the MFMAs of F32X3.  Values must stay inside the
 * fp16 range: BN-scaled weights are checked (|w| < 65504: y3_net_plan / y3_net_forward refuse the mode otherwise),
 * activations are not checked.
 * Y3_DTYPE_F16: the bf16 plan's rules with IEEE fp16 (11 significand bits against bf16's 8) in place of bf16 -- intermediate
 * activations and weights are fp16 (v_mfma_f32_32x32x16_f16 / 16x16x32_f16 at the bf16 rate, fp32 accumulate, BN scale / shift and the
 * shortcut add in fp32, ONE rounding to nearest even where the pipeline stores); the Cin = 3 first layer is fp32 arithmetic storing
 * fp16, the image batch and the head grids stay fp32.  The weights are rounded to fp16 on the host (a further copy of them, 124 MB for
 * YOLOv3, beside the other formats).  Overflow is IEEE's: a value beyond 65504 is stored as inf (as torch.float16 does), a weight
 * beyond it becomes inf; nothing saturates and nothing is checked.  Subnormals are kept.  Same tile ids, heuristic and tuning tables as
 * Y3_DTYPE_BF16 (y3_net_set_tile_bf16); no fused stem unless switched on by y3_net_set_stem_fusion_f16, no split-K unless switched on by
 * y3_net_set_low_latency_f16 / y3_net_set_split_k_f16 (the fp32 / bf16 switches do not act on an fp16 plan).  Head logits measured 8 x closer to fp32 than bf16's
 * (DESIGN.md section 7).
 * In the non-fp32 modes an output tensor that another op of the net reads again, or that a residual conv writes,
 * is kept in the arena in the mode's format and converted into the caller's fp32 buffer at the end of the forward. */
y3_status y3_net_plan(y3_net *net, int max_batch, int image_size, int dtype);

/* The same for a rectangular canvas: batches of height x width inputs (the reference model is Input(shape=(None, None, 3)) and
 * fully convolutional: core/parse_model.py:279-314).  Both sides must be divisible by every tensor's `div` (32 for YOLOv3),
 * otherwise Y3_ERR_INVALID with a message.  y3_net_plan(net, b, S, dtype) IS y3_net_plan_hw(net, b, S, S, dtype): one code path,
 * square results are unchanged bit for bit.  Every call on a planned net (y3_net_forward, y3_net_forward_decode, y3_net_detect,
 * y3_net_read_tensor, y3_net_flops_per_image, y3_net_profile_convs, the measure_sclk calls) follows the planned geometry:
 * images_dev is [B,height,width,3], head grid s is [B, height/div_s, width/div_s, 3*(5+nc)], N = 3 * sum gh_s * gw_s.  The
 * decode inside y3_net_forward_decode / y3_net_detect is y3_yolo_decode_scores_hw below (per-axis normalisation); anchors are
 * normalised (w, h): the caller divides w by the canvas width and h by the canvas height.  The fused stem (y3_net_set_stem_fusion)
 * and the fused head decode serve rectangular plans like square ones.  No tile was tuned for a rectangular plan.
 *
 * A refused or failed call on a planned net leaves one of two states, never a third:
 *   (a) the old plan intact -- nothing was touched, the next forward has the bits of the one before;
 *   (b) no plan -- the old one is freed, y3_net_get_plan answers 0 and every call that needs a plan says "call y3_net_plan first".
 *     refusal                                                                      status          leaves
 *     bad argument, unknown dtype                                                  Y3_ERR_INVALID  (a)
 *     a max-pool net in Y3_DTYPE_F32X3 / _F32X2 / _I8                              Y3_ERR_INVALID  (a)
 *     a side not divisible by a tensor's div                                       Y3_ERR_INVALID  (a)
 *     Y3_DTYPE_F32X2 with a BN-scaled weight outside the fp16 range                Y3_ERR_INVALID  (a)
 *     Y3_DTYPE_I8 with no qualifying conv, or unequal scales at a concat           Y3_ERR_INVALID  (b)
 *     Y3_DTYPE_I8 without a scale it needs                                         Y3_ERR_STATE    (b)
 *     a conv without a tile in the mode                                            Y3_ERR_INVALID  (b)
 *     a tensor of 4 GiB or more (refused before anything is allocated)             Y3_ERR_INVALID  (b)
 *     out of memory (arena, int8 copies, detect scratch, split-K workspace)        Y3_ERR_OOM      (b)
 *     any other failure once the old plan is freed (a HIP error, an exception)     its own         (b)
 * y3_net_get_plan: 1 and the planned max_batch, height, width and dtype (null pointers are skipped) of a planned net; 0 and 0, 0, 0,
 * Y3_DTYPE_F32 without a plan.  A caller that mirrors the plan (Net.max_batch / canvas) asks it after a failed call.
 * A plan is a set of device addresses.  A hipGraph captured from a forward holds the addresses of the plan it was captured on: after
 * another y3_net_plan (or a refusal of kind (b)) those are freed, nothing in the graph or in the library can detect that, and
 * replaying it is undefined.  Capture again after every plan. */
y3_status y3_net_plan_hw(y3_net *net, int max_batch, int height, int width, int dtype);
int y3_net_get_plan(const y3_net *net, int *max_batch, int *height, int *width, int *dtype);

/* images_dev [B,S,S,3] fp32 -> grids_dev[3], each [B,g,g,3*(5+nc)] fp32 (== [B,g,g,3,5+nc]).
 * Replaces model(inputs) (reference: inference.py:109). */
y3_status y3_net_forward(y3_net *net, const float *images_dev, int batch, float *const grids_dev[3], void *stream);

/* debugging / tests: copy images [0, batch) of tensor `tensor_id` of the last forward to dst_dev as fp32 (element count returned
 * through *n_elems; dst_dev may be NULL to query the size).  batch outside 1..max_batch is refused with Y3_ERR_INVALID, the size
 * query included.  The net remembers the (batch, lanes) of the last forward enqueued on the plan: after a forward on one lane any
 * batch up to max_batch reads image i at i * image bytes (images beyond that forward's batch hold what earlier forwards left); after
 * a forward on several lanes the images lie in the lanes' regions (y3_lane_offset): where those follow one another without a gap the
 * read is the one-lane read; otherwise the images are gathered from the regions, lane by lane, and a batch other than that forward's is
 * refused with Y3_ERR_STATE -- its images are not where a contiguous read would look.  Right after y3_net_plan, before any forward on
 * the new plan, a read (not the size query) is refused with Y3_ERR_STATE as well: the new arena holds nothing of the net's, and the
 * previous plan's tensors are gone with it.
 * y3_net_read_tensor_i8 below follows the same rules for an int8 tensor of the arena. */
y3_status y3_net_read_tensor(y3_net *net, int tensor_id, int batch, float *dst_dev, size_t *n_elems, void *stream);

/* ------------------------------------------------------------------------------------------
 * int8 plans (Y3_DTYPE_I8): post-training quantisation, calibrated by the caller.
 * Format: symmetric int8 in [-127, 127]; one fp32 scale s_t per activation tensor (set here), one fp32 scale s_w[c] per output
 * channel of a conv's weights (the library's: y3_net_set_conv_weights quantises the raw conv weights, s_w[c] = absmax_c / 127 or 1 for an
 * all-zero channel, q = clamp(rint(w / s_w[c])) with a true division and round to nearest even; a further copy of the weights, 62 MB for
 * YOLOv3; BN stays in the epilogue).
 * A conv that stores int8 computes, per output element, on exact i32 sums (v_mfma_i32_32x32x32_i8 / v_mfma_i32_16x16x64_i8):
 *     v = (float)acc * sc[c] + sh[c]          two fp32 roundings, never contracted; sc[c] = (s_in * s_w[c]) * bn_scale[c], sh the fp32 plan's shift
 *     v = max(v, 0.1f * v)                    when leaky
 *     v = (float)r * s_res + v                when there is a shortcut; r the int8 shortcut value
 *     q = clamp(rintf(v * (1.0f / s_out)), -127, 127)
 * and a conv that writes an fp32 grid (the heads) stores v = (float)acc * (s_in * s_w[c]) + bias[c].  Every stored byte and every head
 * logit is a fixed function of the input bytes: yolo_v3_tf2_amd/quant.py restates it in NumPy and the tests compare with no tolerance.
 * Where int8 starts: the plan finds the first conv c* in op order such that it and every conv after it has Cin % 128 == 0 (both parts of
 * a concat), and Cout % 16 == 0 unless it writes an fp32 output (YOLOv3: conv 9; 87 % of the FLOPs are behind it).  The convs before c*
 * launch exactly what a Y3_DTYPE_F16 plan launches (y3_net_set_stem_fusion_f16 acts on them); every tensor written before the cut and read
 * behind it gets an int8 copy from one elementwise launch, q = clamp(rintf((float)x * (1.0f / s_t))) (YOLOv3: conv 8's output); an input
 * that feeds an MFMA conv directly (layer tests) is handed over as fp16 and quantised the same way.  A graph with no qualifying conv is
 * refused (Y3_ERR_INVALID), a plan that needs an unset scale is refused with Y3_ERR_STATE naming the tensor, and the two sources of a
 * concat conv must carry the same scale (Y3_ERR_INVALID naming the conv).
 * Tiles: the bf16 table's ids for the tiles that have an int8 form (y3_tile_built(Y3_DTYPE_I8, id): 8, 10, 11, 12, 17, 19, 24, 26, 27,
 * 29), chosen by the bf16 heuristic; y3_net_set_tile_bf16 forces one (a forced tile without an int8 form leaves the conv to the
 * heuristic).  No int8 tuning table is shipped.  y3_net_forward_decode / y3_net_detect decode the heads in the launch as in a bf16 plan.
 * Split-K: y3_net_set_low_latency_i8 / y3_net_set_split_k_i8 above (the fp32, bf16 and fp16 switches do not act on an int8 plan).
 * Not in this version: a weight-resident tile, BK = 32 tiles (so no int8 for Cin = 32 / 64), split forms of the 16x16x64 and 16-wave
 * tiles, and the int8 copy fused into the producing epilogue.
 *
 * y3_net_set_act_scales: n_tensors must be the net's tensor count; entries <= 0 mean unset.  Read by the next y3_net_plan: on a planned
 * int8 net it waits for it (the plan in force keeps the scales it took, also for weights loaded later).
 * y3_net_get_act_scale: the scale set for a tensor, 0 when unset.  y3_net_i8_first_conv: c* of a net planned in Y3_DTYPE_I8, else -1.
 * y3_net_read_tensor_i8: the raw bytes of an int8 tensor of the last forward (a tensor behind the cut, or the int8 copy of one that
 * crosses it); y3_net_read_tensor on an int8 tensor returns (float)q * s.
 *
 * Stand-alone ops in int8 (YOLOv3-tiny), a switch of its own: y3_net_set_pools_i8(net, 1), off by default and read by the next
 * y3_net_plan (a planned net keeps its plan).  Off: an int8 plan refuses a net that holds a max-pool, and runs no stand-alone op behind
 * its cut.  On, in a Y3_DTYPE_I8 plan (it does nothing in any other): the cut is found as before, from the convs alone; a tensor is
 * behind the cut when a conv at or after the cut or an int8 aux op writes it; walking the aux ops in op order, a max-pool (either
 * stride), an up-sample or a concat whose every source is behind the cut runs in int8 -- the pool through y3_maxpool2x2's kernel on signed
 * bytes, the other two as moves of bytes -- and its destination is an int8 tensor; an aux op none of whose sources is behind the cut runs as
 * in an fp16 plan.  Such an op only selects or moves stored bytes, so its destination and all its sources must carry ONE scale: unequal
 * scales are refused with Y3_ERR_INVALID naming the op, the tensors and the values, a missing one with Y3_ERR_STATE naming the tensor
 * (the quantiser is monotone, so a pool of quantised values is the quantised pool, byte for byte).  Refused by name with Y3_ERR_INVALID,
 * and with the plan in force left as it is: a concat with one source behind the cut and one before it, a stand-alone add with a source
 * behind the cut, an aux op behind the cut that reads a net output, an int8 aux op with a channel count that is no multiple of 16.  A
 * tensor written before the cut by a conv or an aux op and read by an int8 conv gets its int8 copy as before (tiny: pool 3's output, tensor
 * 8).  The part before the cut is an fp16 plan bit for bit: YOLOv3-tiny needs y3_net_set_tiny_stem_fusion as well (its 32 -> 32 conv has
 * no fp16 tile), and the fused tiny stem then runs in its fp16 form.  y3_net_pools_i8: 1 when the plan in force runs at least one aux op in
 * int8, else 0 (no plan, a null net). */
y3_status y3_net_set_pools_i8(y3_net *net, int on);
int y3_net_pools_i8(const y3_net *net);
y3_status y3_net_set_act_scales(y3_net *net, const float *scales, int n_tensors);
float y3_net_get_act_scale(const y3_net *net, int tensor_id);
int y3_net_i8_first_conv(const y3_net *net);
y3_status y3_net_read_tensor_i8(y3_net *net, int tensor_id, int batch, int8_t *dst_dev, size_t *n_elems, void *stream);

/* conv FLOPs (2*MAC) of one image at the planned size (height x width) */
double y3_net_flops_per_image(const y3_net *net);

/* Time every conv launch of one forward (hipEvents on `stream`); ms_out[n_convs]. Synchronises. */
y3_status y3_net_profile_convs(y3_net *net, const float *images_dev, int batch, float *ms_out, int n, void *stream);

/* ------------------------------------------------------------------------------------------
 * Image input stage (the step right before the path): decode_image(channels=3, dtype=float32) + tf.image.resize
 * (reference: inference.py:157-158).  image_dev: [height,width,channels] uint8 (is_uint8=1; converted with * 1/255) or
 * float32 (is_uint8=0); channels 3 or 4 (alpha dropped).  is_uint8=2 is the tfrecords source's order of operations
 * (reference: core/load_tfrecords.py:46-48): uint8 taken as 0..255, resized, then divided by 255.  Writes the bilinear (half-pixel centres, no antialias)
 * resize to image_size x image_size into batch_dev[slot] of an NHWC fp32 batch [*,image_size,image_size,3].
 *
 * Y3_IMAGE_LETTERBOX, OR-ed into is_uint8 (and into y3_image_desc.mode below), keeps the aspect ratio instead: the image is
 * resized to sh x sw and centred on a zero canvas (reference: core/utils.py:17-28, resize_image = tf.image.resize(
 * preserve_aspect_ratio=True) + pad_to_bounding_box).  The geometry {sh, sw, top, left} is, in fp32,
 *   scale = min((float)S / (float)h, (float)S / (float)w)
 *   sh = max(1, (int)nearbyintf(scale * (float)h)), sw = max(1, (int)nearbyintf(scale * (float)w))   (round half to even)
 *   top = (S - sh) / 2, left = (S - sw) / 2                                                           (floor)
 * A pixel inside [top, top + sh) x [left, left + sw) is the bilinear sample of a resize to sh x sw; every other pixel of
 * the slot is written as 0.0f.  A geometry that does not fit the canvas is Y3_ERR_INVALID (pad_to_bounding_box raises).
 * The valid values of is_uint8 / mode are 0, 1, 2, each with or without the flag.
 * ---------------------------------------------------------------------------------------- */
#define Y3_IMAGE_LETTERBOX 0x100
y3_status y3_preprocess_image(const void *image_dev, int is_uint8, int height, int width, int channels,
                              float *batch_dev, int slot, int image_size, void *stream);
/* The same onto a canvas_h x canvas_w canvas (batch_dev is [*,canvas_h,canvas_w,3]).  Without the flag the image is stretched to
 * canvas_h x canvas_w.  With it the geometry is, in fp32,
 *   scale = min((float)canvas_h / (float)h, (float)canvas_w / (float)w)
 *   sh, sw as above;  top = (canvas_h - sh) / 2, left = (canvas_w - sw) / 2
 * y3_preprocess_image(..., S, stream) IS y3_preprocess_image_hw(..., S, S, stream).  Same argument checks. */
y3_status y3_preprocess_image_hw(const void *image_dev, int is_uint8, int height, int width, int channels,
                                 float *batch_dev, int slot, int canvas_h, int canvas_w, void *stream);

/* The same stage for a batch of unlike images in one launch per 72 images (no reference counterpart: the reference resizes
 * image by image).  All images lie in ONE device blob `pixels_dev` of `pixels_bytes` bytes; image i starts `offset` bytes into
 * it, is [height,width,channels] (channels 3 or 4, alpha dropped) and has `mode` with the meaning of is_uint8 above: 0 float32
 * (offset and pixels_dev 4-byte aligned), 1 uint8 * 1/255 before the resize, 2 uint8 divided by 255 after it, each optionally
 * OR-ed with Y3_IMAGE_LETTERBOX (per image: one batch may mix stretched and letterboxed images).  Image i is
 * written to batch_dev[first_slot + i]; every value is bit-identical to the per-image call.  descs_host is read during the call (the
 * descriptors travel in the kernel arguments), so the caller may reuse it at once.  All arguments are checked on the host
 * before anything is enqueued (Y3_ERR_INVALID names the index of the bad image); the call only enqueues on `stream`: it does
 * not allocate, query or synchronise, and can be captured into a HIP graph (the descriptors are then frozen into it). */
typedef struct y3_image_desc { uint64_t offset; int32_t height, width, channels, mode; } y3_image_desc;
y3_status y3_preprocess_batch(const void *pixels_dev, size_t pixels_bytes, const y3_image_desc *descs_host, int n_images,
                              float *batch_dev, int first_slot, int image_size, void *stream);
/* ... onto a canvas_h x canvas_w canvas; the square call is this one with canvas_h == canvas_w.  Same checks, same messages. */
y3_status y3_preprocess_batch_hw(const void *pixels_dev, size_t pixels_bytes, const y3_image_desc *descs_host, int n_images,
                                 float *batch_dev, int first_slot, int canvas_h, int canvas_w, void *stream);

/* The letterbox geometry of a batch, on the host (no HIP call): geoms_out_host[n_images][4] = {sh, sw, top, left} by the
 * formula above, from height / width / mode of each descriptor (offset and channels are not read); an image without
 * Y3_IMAGE_LETTERBOX gets {image_size, image_size, 0, 0}.  y3_preprocess_batch and y3_preprocess_image compute their
 * geometries with the same routine.  One call per batch. */
y3_status y3_letterbox_geometry(const y3_image_desc *descs_host, int n_images, int image_size, int32_t *geoms_out_host);
/* ... for a canvas_h x canvas_w canvas (y3_preprocess_image_hw gives the formula); without the flag {canvas_h, canvas_w, 0, 0}. */
y3_status y3_letterbox_geometry_hw(const y3_image_desc *descs_host, int n_images, int canvas_h, int canvas_w, int32_t *geoms_out_host);

/* ------------------------------------------------------------------------------------------
 * yolo_decode   (reference: core/yolo_decode_layer.py:15-36)
 * grids_dev[s]: [B,g_s,g_s,3,5+nc]; anchors_host: [3][3][2] normalised (w,h), scale s uses anchors[s].
 * Outputs [B,N,4], [B,N,1], [B,N,nc] with N = 3*sum g_s^2, scales concatenated in input order.
 * ---------------------------------------------------------------------------------------- */
y3_status y3_yolo_decode(const float *const grids_dev[3], const int32_t grid_sizes[3], int batch, int nclasses,
                         const float *anchors_host, float *bboxes_dev, float *conf_dev, float *probs_dev,
                         void *stream);

/* decode fused with the class arg-max / score of yolo_nms (reference: core/yolo_nms.py:18-24):
 * writes bboxes [B,N,4], class_indices [B,N] int64, scores [B,N]; class probabilities are not stored. */
y3_status y3_yolo_decode_scores(const float *const grids_dev[3], const int32_t grid_sizes[3], int batch,
                                int nclasses, const float *anchors_host, float *bboxes_dev,
                                int64_t *class_idx_dev, float *scores_dev, void *stream);

/* The two decodes for rectangular grids: grid_hw[s] = {gh_s, gw_s}, grids_dev[s] is [B,gh_s,gw_s,3,5+nc], N = 3 * sum gh_s * gw_s.
 * Row order as above: n = off_s + (row * gw_s + col) * 3 + a.  Each centre is normalised by the extent of ITS OWN axis:
 *   x = (sigmoid(tx) + col) / (float)gw      y = (sigmoid(ty) + row) / (float)gh
 * so that boxes are normalised (xmin,ymin,xmax,ymax) of the gh x gw canvas.  This is a DELIBERATE departure from the reference
 * for gh != gw: its __arrange_bbox (core/yolo_decode_layer.py:5-8) divides (x, y) by cast(shape[1:3]) = (gh, gw) -- x by the
 * number of rows -- and oracle/y3_oracle.c:162-163 restates exactly that.  The two coincide for every square grid, which is all
 * the reference ever runs; for other grids the reference's result is not a normalised coordinate.  y3_yolo_decode /
 * y3_yolo_decode_scores ARE these calls with {g, g}: the same kernel body, square results unchanged bit for bit.
 * Anchors stay normalised (w, h): the caller normalises w by the canvas width and h by the canvas height.
 * Host restatement: core/yolo_decode_layer.yolo_decode_hw_host. */
y3_status y3_yolo_decode_hw(const float *const grids_dev[3], const int32_t grid_hw[3][2], int batch, int nclasses,
                            const float *anchors_host, float *bboxes_dev, float *conf_dev, float *probs_dev,
                            void *stream);
y3_status y3_yolo_decode_scores_hw(const float *const grids_dev[3], const int32_t grid_hw[3][2], int batch,
                                   int nclasses, const float *anchors_host, float *bboxes_dev,
                                   int64_t *class_idx_dev, float *scores_dev, void *stream);

/* The decodes for n_scales grids, 1 <= n_scales <= 3 (two for YOLOv3-tiny): grids_dev[n_scales], grid_hw[n_scales][2], anchors_host
 * [n_scales][3][2], N = 3 * sum over those scales of gh_s * gw_s; nothing behind entry n_scales - 1 of an array is read.  These are the
 * one body: y3_yolo_decode_hw / y3_yolo_decode_scores_hw ARE these calls with 3, the square forms those with {g, g}. */
y3_status y3_yolo_decode_hw_n(const float *const *grids_dev, const int32_t (*grid_hw)[2], int n_scales, int batch, int nclasses,
                              const float *anchors_host, float *bboxes_dev, float *conf_dev, float *probs_dev, void *stream);
y3_status y3_yolo_decode_scores_hw_n(const float *const *grids_dev, const int32_t (*grid_hw)[2], int n_scales, int batch, int nclasses,
                                     const float *anchors_host, float *bboxes_dev, int64_t *class_idx_dev, float *scores_dev,
                                     void *stream);

/* ------------------------------------------------------------------------------------------
 * MaxPooling2D(pool_size = 2, strides = stride, padding = 'same'), stride 1 or 2 (reference: core/parse_model.py:78-99), the pools of
 * YOLOv3-tiny.  src_dev [batch,H,W,C] -> dst_dev [batch,H/stride,W/stride,C], NHWC, elements of `dtype`: Y3_DTYPE_F32 (fp32),
 * Y3_DTYPE_BF16 or Y3_DTYPE_F16 (2 bytes), or Y3_DTYPE_I8 (signed bytes, all 256 values legal, each byte compared on its own);
 * C * element size must be a multiple of 16 bytes, both pointers 16-byte aligned.
 *   stride 2 (H and W even): out[y, x] = max over in[2y .. 2y + 1, 2x .. 2x + 1]
 *   stride 1: 'same' pads one row below and one column to the right and padding never wins, so
 *             out[y, x] = max over in[y .. min(y + 1, H - 1), x .. min(x + 1, W - 1)]
 * Elements are compared as values and the winning element's bits are stored.  What a window holding a NaN gives, and the sign of a
 * result that is zero when the window holds both -0 and +0, are unspecified.  TensorFlow's own kernel is not pinned by this project's
 * tests; yolo_v3_tf2_amd/maxpool.py restates the rule in NumPy.  Only enqueues on `stream`: no allocation, query or synchronisation, so
 * it can be captured into a HIP graph.  A net runs the same kernel for its Y3_AUX_MAXPOOL2X2_* ops, per lane slice.
 * ---------------------------------------------------------------------------------------- */
y3_status y3_maxpool2x2(const void *src_dev, void *dst_dev, int batch, int height, int width, int channels, int stride, int dtype,
                        void *stream);

/* ------------------------------------------------------------------------------------------
 * yolo_nms / YoloNmsLayer.call   (reference: core/yolo_nms.py:16-34, core/yolo_nms_layer.py:26-29)
 * ---------------------------------------------------------------------------------------- */
/* class_indices = argmax(probs), scores = conf * max(probs)   (core/yolo_nms.py:18-24) */
y3_status y3_class_scores(const float *conf_dev, const float *probs_dev, int batch, int n, int nclasses,
                          int64_t *class_idx_dev, float *scores_dev, void *stream);

/* bytes of scratch y3_nms_padded needs for (batch, n) */
size_t y3_nms_workspace_bytes(int batch, int n);

/* tf.image.non_max_suppression_padded(boxes[B,N,4], scores[B,N], max_output_size, iou_threshold,
 * score_threshold, pad_to_max_output_size=True)   (core/yolo_nms.py:26-33)
 * -> selected_idx [B,max_output_size] int32 (zero padded), num_valid [B] int32. */
y3_status y3_nms_padded(const float *bboxes_dev, const float *scores_dev, int batch, int n, int max_output_size,
                        float iou_threshold, float score_threshold, int32_t *selected_idx_dev,
                        int32_t *num_valid_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* Per-class NMS (no reference counterpart; off by default everywhere).  The rule of y3_nms_padded with one predicate changed: a
 * candidate is suppressed by an earlier kept candidate iff their class ids are equal AND IoU >= iou_threshold (the same fp32 IoU,
 * the arguments in the same order).  Everything else is y3_nms_padded's: scores <= score_threshold are masked out, the
 * canonicalisation is decided by box [0,0] of the batch, the order is (score descending, index ascending) with -0 == +0, a box is
 * selected iff any of its coordinates is > 0, and the first max_output_size selected boxes OVER ALL CLASSES TOGETHER are returned in
 * sorted order, the rest of the row zero, num_valid = min(count, max_output_size).  With all class ids equal the outputs are those
 * of y3_nms_padded bit for bit.  class_idx_dev: int64 [batch,n] as y3_class_scores / y3_net_forward_decode write it; the ids are
 * compared as int32 and must lie in [0, 2^31).  iou_threshold <= 0 (the tile quirk of the agnostic rule) has no meaning here and is
 * refused with Y3_ERR_INVALID; the other argument checks are y3_nms_padded's.  The workspace holds the class ids of spilled kept
 * boxes as well: y3_nms_per_class_workspace_bytes = y3_nms_workspace_bytes + batch * n * 4.  Only enqueues: may be captured. */
size_t y3_nms_per_class_workspace_bytes(int batch, int n);
y3_status y3_nms_padded_per_class(const float *bboxes_dev, const float *scores_dev, const int64_t *class_idx_dev, int batch, int n,
                                  int max_output_size, float iou_threshold, float score_threshold, int32_t *selected_idx_dev,
                                  int32_t *num_valid_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* Inference.gather_valid_detections_results for a whole batch (reference: inference.py:21-28), packed for the
 * multi-GPU exchange: per image max_out rows of {box[4], score, class (int32), index (int32)} = 7 x 4 bytes
 * (rows >= num_valid zeroed), i.e. packed_dev is [B,max_out,7] of 32-bit words. */
y3_status y3_pack_detections(const float *bboxes_dev, const int64_t *class_idx_dev, const float *scores_dev,
                             const int32_t *selected_idx_dev, const int32_t *num_valid_dev, int batch, int n,
                             int max_out, void *packed_dev, void *stream);

/* Conv program + decode in one call: images -> (bboxes [B,N,4], class_indices [B,N] int64, scores [B,N]), i.e.
 * model(inputs) -> yolo_decode -> argmax / score (reference: inference.py:109-117 up to the NMS; core/yolo_decode_layer.py:15-36,
 * core/yolo_nms.py:18-24).  Where the graph allows it (every head a 1x1 conv + bias writing its grid; fp32 and bf16 plans) the
 * three head convs decode their own output tiles while these are still on chip, and the [B,g,g,3*(5+nc)] grids are neither
 * written nor read back; otherwise it is y3_net_forward into net-owned scratch + y3_yolo_decode_scores.  Either way the
 * results are bit-identical to that composed route.  Outputs are caller-owned device buffers; bboxes 16-byte aligned. */
y3_status y3_net_forward_decode(y3_net *net, const float *images_dev, int batch, const float *anchors_host, float *bboxes_dev,
                                int64_t *class_idx_dev, float *scores_dev, void *stream);
/* ------------------------------------------------------------------------------------------
 * The whole path in one call: Model(inputs, nms_output).predict(batch) followed by the per-image gather
 * (reference: inference.py:109-117, 125-128, 21-28) = y3_net_forward -> y3_yolo_decode_scores -> y3_nms_padded ->
 * y3_pack_detections on net-owned scratch.  images_dev [batch,S,S,3] fp32; anchors_host [3][3][2];
 * packed_dev [batch,max_boxes,7] 32-bit words {xmin,ymin,xmax,ymax,score,class(int32),index(int32)}, rows >= num_valid
 * zeroed; num_valid_dev [batch] int32.  max_boxes in [1,1024].  Everything is enqueued on `stream`: the scratch (grids,
 * decoded tensors, NMS workspace) is allocated by y3_net_plan for max_batch images, so the call allocates nothing and
 * may be the first thing captured into a HIP graph.
 * ---------------------------------------------------------------------------------------- */
y3_status y3_net_detect(y3_net *net, const float *images_dev, int batch, const float *anchors_host, int max_boxes,
                        float iou_threshold, float score_threshold, void *packed_dev, int32_t *num_valid_dev,
                        void *stream);
/* y3_net_detect for callers that want the raw head grids as well (the validation loss reads them): grids_out_dev as y3_net_forward's
 * grids_dev, three caller-owned fp32 buffers, 16-byte aligned, written exactly as y3_net_forward writes them.  The decode is then the
 * stand-alone one over those grids (y3_yolo_decode_scores_hw; y3_yolo_decode_candidates_hw in multi-label mode) -- the composed route, to
 * which y3_net_detect is bit-identical, so packed_dev and num_valid_dev are y3_net_detect's bit for bit.  y3_net_detect is this call
 * without the grids: the same checks, the same scratch, the same NMS mode and multi-label switch, and every check comes before the first
 * launch -- a refused call of either enqueues nothing. */
y3_status y3_net_detect_grids(y3_net *net, const float *images_dev, int batch, const float *anchors_host, int max_boxes,
                              float iou_threshold, float score_threshold, float *const grids_out_dev[3], void *packed_dev,
                              int32_t *num_valid_dev, void *stream);
/* Which NMS rule y3_net_detect enqueues: Y3_NMS_AGNOSTIC (the default: y3_nms_padded, the reference's rule) or Y3_NMS_PER_CLASS
 * (y3_nms_padded_per_class on the class ids of the decode; iou_threshold must then be > 0).  Read when y3_net_detect enqueues: a
 * captured graph keeps the mode it was captured in.  y3_net_plan reserves the larger workspace, so the mode may be switched
 * after planning.  Nothing else about y3_net_detect changes: the packed rows keep their format. */
enum { Y3_NMS_AGNOSTIC = 0, Y3_NMS_PER_CLASS = 1 };
y3_status y3_net_set_nms_mode(y3_net *net, int mode);
int y3_net_get_nms_mode(const y3_net *net);

/* ------------------------------------------------------------------------------------------
 * Multi-label detections (no reference counterpart; Darknet's detector and the published YOLOv3 protocol): every pair (box n,
 * class c) with conf[n] * prob[n,c] > score_threshold is a candidate of its own, and the NMS decides between candidates.
 * bboxes / conf / prob are those of y3_yolo_decode_hw bit for bit (the same per-box body), the score is one fp32 multiply -- the
 * expression of y3_yolo_decode_scores, so the score of a box's arg-max class is its single-label score bit for bit.  The test is
 * strict (the complement of the NMS's "scores <= S are masked out"); a NaN score is no candidate; with score_threshold < 0 every
 * pair with a non-NaN score is one.  The candidates of image b are numbered k = 0, 1, ... in the order (n ascending, c ascending);
 * that order is part of the rule (the NMS breaks score ties by index) and comes from counts and prefix sums, never from the
 * arrival order of workgroups or atomics.  totals_dev [batch] int32: the number of candidates of each image, uncapped; the first
 * min(total, capacity) are stored: cand_boxes_dev [batch,capacity,4] f32 (16-byte aligned) = bboxes[n], cand_cls_dev
 * [batch,capacity] int64 = c, cand_scores_dev [batch,capacity] f32, cand_src_dev [batch,capacity] int32 = n.  Rows
 * k >= min(total, capacity) are box (0,0,0,0), score 0, class 0, source 0 (the filler of y3_merge_tile_detections: the padded NMS never
 * selects such a row).  Every word of the five arrays is written on every call; total[b] > capacity says image b was truncated.
 * workspace_dev: y3_decode_candidates_workspace_bytes bytes (one int32 per box; 0: bad arguments), 4-byte aligned.
 * Checked before the first launch -- a refused call enqueues nothing: null pointers; batch, capacity, nclasses >= 1; grids and
 * cand_boxes 16-byte aligned; batch * capacity and N * nclasses below 2^31; the workspace; 64 * (5 + nclasses) * 4 bytes of LDS
 * within 160 KB.  Three launches (count, per-image prefix, write); only enqueues: may be captured.
 * Downstream is what exists: y3_nms_padded_per_class / y3_nms_padded over [batch,capacity], then y3_pack_detections, then
 * y3_candidate_sources, which rewrites the index word (word 6) of every valid packed row from k to cand_src[b,k] -- a multi-label
 * row reads {box of n, score[n,c], c, n} and two rows of one image may share n.
 * ---------------------------------------------------------------------------------------- */
size_t y3_decode_candidates_workspace_bytes(const int32_t grid_hw[3][2], int batch, int nclasses);
/* ... for n_scales grids (1..3), as y3_yolo_decode_hw_n: the three-scale names above and below ARE these calls with 3. */
size_t y3_decode_candidates_workspace_bytes_n(const int32_t (*grid_hw)[2], int n_scales, int batch, int nclasses);
y3_status y3_yolo_decode_candidates_hw_n(const float *const *grids_dev, const int32_t (*grid_hw)[2], int n_scales, int batch, int nclasses,
                                         const float *anchors_host, float score_threshold, int capacity, float *cand_boxes_dev,
                                         int64_t *cand_cls_dev, float *cand_scores_dev, int32_t *cand_src_dev, int32_t *totals_dev,
                                         void *workspace_dev, size_t workspace_bytes, void *stream);
y3_status y3_yolo_decode_candidates_hw(const float *const grids_dev[3], const int32_t grid_hw[3][2], int batch, int nclasses,
                                       const float *anchors_host, float score_threshold, int capacity, float *cand_boxes_dev,
                                       int64_t *cand_cls_dev, float *cand_scores_dev, int32_t *cand_src_dev, int32_t *totals_dev,
                                       void *workspace_dev, size_t workspace_bytes, void *stream);
/* The same rule for callers that hold the decoded tensors, as y3_class_scores is to y3_yolo_decode_scores: bboxes_dev [batch,n,4]
 * (16-byte aligned), conf_dev [batch,n], probs_dev [batch,n,nclasses] as y3_yolo_decode writes them -> the same five arrays, bit for
 * bit those of y3_yolo_decode_candidates_hw on the grids they were decoded from.  workspace_dev: batch * n * 4 bytes.  The same
 * checks before the first launch; only enqueues. */
y3_status y3_class_candidates(const float *bboxes_dev, const float *conf_dev, const float *probs_dev, int batch, int n, int nclasses,
                              float score_threshold, int capacity, float *cand_boxes_dev, int64_t *cand_cls_dev, float *cand_scores_dev,
                              int32_t *cand_src_dev, int32_t *totals_dev, void *workspace_dev, size_t workspace_bytes, void *stream);
/* packed_dev [batch,max_boxes,7], num_valid_dev [batch] as y3_pack_detections wrote them over [batch,capacity] candidates; an index
 * word outside [0, capacity) is left alone.  Only enqueues. */
y3_status y3_candidate_sources(void *packed_dev, const int32_t *num_valid_dev, const int32_t *cand_src_dev, int batch, int capacity,
                               int max_boxes, void *stream);
/* y3_net_detect in multi-label mode (off by default; with it off every call enqueues exactly what it enqueued before): y3_net_forward
 * into the net-owned grid scratch, y3_yolo_decode_candidates_hw, the NMS of the net's mode over [batch,K], y3_pack_detections,
 * y3_candidate_sources.  capacity 0: K = N of the plan; otherwise 1 <= capacity <= N, so that the candidates and the NMS live in the
 * scratch y3_net_plan reserves for N boxes (a capacity above the planned N is refused with Y3_ERR_INVALID when y3_net_detect
 * enqueues).  y3_net_plan always reserves the sources, totals and counts besides, so the switch may be flipped after planning; it is
 * read when y3_net_detect enqueues, and a captured graph keeps what it was captured with.  Every plan dtype writes fp32 grids, so
 * every one works.  y3_net_read_multi_label_totals enqueues a copy of the totals of the first `batch` images of the last
 * multi-label detect enqueued on this plan (Y3_ERR_STATE: none was) into dst_dev [batch] int32, batch <= max_batch; images that detect did not have read 0. */
y3_status y3_net_set_multi_label(y3_net *net, int on, int capacity);
int y3_net_get_multi_label(const y3_net *net);
int y3_net_get_multi_label_capacity(const y3_net *net);
y3_status y3_net_read_multi_label_totals(y3_net *net, int batch, int32_t *dst_dev, void *stream);

/* Packed detections of letterboxed images -> coordinates of the source frames, in place (no reference counterpart: the
 * reference leaves its boxes on the padded canvas).  packed_dev [batch,max_boxes,7] and num_valid_dev [batch] as written by
 * y3_net_detect / y3_pack_detections; geoms_host [batch][4] = {sh, sw, top, left} as y3_letterbox_geometry gives them, read
 * during the call (they travel in the kernel arguments, 64 images per launch).  For every row r < num_valid[b], in fp32,
 * each operation rounded on its own:
 *   xmin' = (xmin * (float)S - (float)left) / (float)sw      xmax' likewise
 *   ymin' = (ymin * (float)S - (float)top) / (float)sh       ymax' likewise
 * Boxes are not clipped (the reference never clips).  Score, class and index words, rows >= num_valid, and every row of an
 * image whose geometry is {S, S, 0, 0} are not touched.  The geometries (1 <= sh, sw; 0 <= top, left; top + sh <= S,
 * left + sw <= S) and max_boxes in [1,1024] are checked on the host before anything is enqueued (Y3_ERR_INVALID names the
 * bad image); the call only enqueues on `stream` -- no allocation, query or synchronise -- and can be captured. */
y3_status y3_unletterbox_detections(void *packed_dev, const int32_t *num_valid_dev, const int32_t *geoms_host, int batch,
                                    int max_boxes, int image_size, void *stream);
/* ... for a canvas_h x canvas_w canvas (geometries of y3_letterbox_geometry_hw):
 *   x' = (x * (float)canvas_w - (float)left) / (float)sw      y' = (y * (float)canvas_h - (float)top) / (float)sh
 * an image whose geometry is {canvas_h, canvas_w, 0, 0} is not touched.  The square call is this one with canvas_h == canvas_w. */
y3_status y3_unletterbox_detections_hw(void *packed_dev, const int32_t *num_valid_dev, const int32_t *geoms_host, int batch,
                                       int max_boxes, int canvas_h, int canvas_w, void *stream);

/* ------------------------------------------------------------------------------------------
 * Sliced inference (no reference counterpart; nothing here runs unless it is called): a large frame is cut into overlapping
 * windows, every window goes through the network as an image of its own, and the windows' detections are mapped back to the frame
 * and merged by a second NMS.  Host restatements: tiles.tile_grid, tiles.merge_tile_detections_ref.
 * ---------------------------------------------------------------------------------------- */
/* The windows of a height x width frame, on the host, integers only: out[T][4] = {y0, x0, ch, cw}, rows x cols windows in
 * row-major order and, with overview != 0, the whole frame {0, 0, height, width} LAST.  Per axis, with extent e, count k and
 * ov = overlap_px:
 *   len = ceil_div(e + (k - 1) * ov, k)          origin of window i = floor(i * (e - len) / (k - 1)), 0 when k == 1
 * so that every window lies inside the frame, the windows cover it, the first starts at 0, the last ends at e and neighbours
 * overlap by at least ov.  Returns T = rows * cols + (overview ? 1 : 0), or -1 (with y3_last_error) for what it refuses: a null
 * `out`, height or width < 1, rows or cols outside [1,8], ov < 0, ov > min(height, width), T > 64. */
int y3_tile_grid(int height, int width, int rows, int cols, int overlap_px, int overview, int32_t *out);

/* y3_preprocess_batch_hw for windows of images: tile i is the window [y0, y0 + ch) x [x0, x0 + cw) of the
 * height x width x channels image that starts `offset` bytes into pixels_dev, and is treated AS AN IMAGE OF ITS OWN: the bilinear
 * taps clamp at the window's edges, and with Y3_IMAGE_LETTERBOX the geometry is that of a ch x cw image.  `mode` as in
 * y3_image_desc.  Tile i is written to batch_dev[first_slot + i], and every value is bit-identical to y3_preprocess_batch_hw on a
 * contiguous copy of the window: the same kernel reads the frame with the frame's row pitch (an image is the whole-frame window of
 * itself).  Several tiles may name the same image, which is therefore uploaded once.  The descriptors travel in the kernel
 * arguments, 72 tiles per launch.  Checked on
 * the host before anything is enqueued (Y3_ERR_INVALID names the tile): everything y3_preprocess_batch checks, ch and cw >= 1,
 * the window inside the image, the letterbox of ch x cw fitting the canvas.  Only enqueues on `stream`; can be captured. */
typedef struct y3_tile_desc { uint64_t offset; int32_t height, width, channels, mode; int32_t y0, x0, ch, cw; } y3_tile_desc;
y3_status y3_preprocess_tiles_hw(const void *pixels_dev, size_t pixels_bytes, const y3_tile_desc *descs_host, int n_tiles,
                                 float *batch_dev, int first_slot, int canvas_h, int canvas_w, void *stream);
/* y3_letterbox_geometry_hw for tiles, on the host: geoms_out_host[n_tiles][4] = {sh, sw, top, left} from (ch, cw) and mode of
 * each descriptor -- the geometry of a ch x cw image; without the flag {canvas_h, canvas_w, 0, 0}. */
y3_status y3_tile_letterbox_geometry_hw(const y3_tile_desc *descs_host, int n_tiles, int canvas_h, int canvas_w, int32_t *geoms_out_host);

/* The tiles' packed rows -> one packed result per frame.  packed_dev [frames*tiles,max_boxes,7] and num_valid_dev [frames*tiles]
 * are what y3_net_detect leaves on the tile batch (tile t of frame f is image f * tiles + t): boxes normalised to the canvas and
 * NOT un-letterboxed.  tiles_host [frames*tiles][4] = {y0, x0, ch, cw} (y3_tile_grid), geoms_host [frames*tiles][4] =
 * {sh, sw, top, left} (y3_tile_letterbox_geometry_hw), frame_hw_host [frames][2] = {h, w}; all three are read during the call
 * (they travel in the kernel arguments, 64 tile images per launch).
 * merge_tiles_kernel writes three candidate arrays per frame into the workspace, candidate n = t * max_boxes + r: boxes
 * [frames,tiles*max_boxes,4], scores [frames,tiles*max_boxes], class ids int64 [frames,tiles*max_boxes].  For a row
 * r < num_valid (clamped to [0,max_boxes]), per axis in fp32, every operation rounded on its own:
 *   u  = (x * (float)canvas_w - (float)left) / (float)sw        u = x where sw == canvas_w and left == 0
 *   x' = ((float)x0 + u * (float)cw) / (float)w                 x' = u where x0 == 0 and cw == w
 * and y likewise with sh, top, canvas_h, y0, ch, h.  u is the expression of y3_unletterbox_detections_hw, but the identity is
 * decided PER AXIS here (there the whole geometry decides: an axis that fills the canvas of a letterboxed image is computed as
 * x * W / W, which need not be x).  Score and class are copied; nothing is clipped.  A row r >= num_valid becomes box 0, score 0,
 * class 0, which the padded NMS never selects; every word of the three arrays is written.
 * Then, on the same stream and on those arrays, the existing y3_nms_padded(frames, tiles*max_boxes, max_boxes, iou_threshold,
 * score_threshold) -- y3_nms_padded_per_class with nms_mode == Y3_NMS_PER_CLASS -- and y3_pack_detections: the merged rows are
 * that rule applied to the union of the tiles' survivors, every quirk of it included (the canonicalisation decided by candidate 0
 * of frame 0, iou_threshold <= 0).  packed_out_dev [frames,max_boxes,7], num_valid_out_dev [frames]; the index word of a merged
 * row is t * max_boxes + r.
 * The workspace (16-byte aligned) holds, each part starting on a multiple of 16 bytes and in this order, the candidate boxes, class ids
 * and scores, the selected indices [frames,max_boxes] and the NMS workspace of (frames, tiles*max_boxes):
 * y3_merge_tiles_workspace_bytes, which serves either mode and is 0 for arguments the call refuses.  Checked on the host before
 * anything is enqueued (Y3_ERR_INVALID names the offender): frames >= 1, tiles in [1,64], max_boxes in [1,1024], frames * tiles *
 * max_boxes < 2^31, the windows inside their frames, the geometries inside the canvas, nms_mode, the threshold checks of the NMS
 * call, the workspace size, the alignment (packed 4 bytes, workspace 16).  Only enqueues on `stream`; can be captured. */
size_t y3_merge_tiles_workspace_bytes(int frames, int tiles, int max_boxes);
y3_status y3_merge_tile_detections(const void *packed_dev, const int32_t *num_valid_dev, const int32_t *tiles_host,
                                   const int32_t *geoms_host, const int32_t *frame_hw_host, int frames, int tiles, int max_boxes,
                                   int canvas_h, int canvas_w, int nms_mode, float iou_threshold, float score_threshold,
                                   void *packed_out_dev, int32_t *num_valid_out_dev, void *workspace_dev, size_t workspace_bytes,
                                   void *stream);

/* ------------------------------------------------------------------------------------------
 * Evaluation counters for every NMS score threshold of a sweep, from ONE detect pass (reference:
 * evaluate_detections.py:37-48,82-135, EvaluateDetections.iou_alg / evaluate; evaluate_yolov3.py:153-232, the loop over
 * evaluate_nms_score_thresholds that the reference runs as one whole pass over the data set per threshold).
 * The greedy padded NMS suppresses a box only by survivors scored above it, so the detections at a higher score threshold are
 * the rows of the lowest threshold's result with score > threshold, in the same order: packed_dev [batch,max_boxes,7] and
 * num_valid_dev [batch] are what y3_net_detect (at the lowest threshold of the sweep), y3_pack_detections or
 * y3_unletterbox_detections leave behind.  Ground truth: gt_boxes_dev [batch,max_gt,4] {xmin,ymin,xmax,ymax}, gt_classes_dev
 * [batch,max_gt] int32, the first gt_count_dev[b] rows of image b (counts are clamped to [0,max_gt], num_valid to [0,max_boxes]).
 * score_thresholds_host [n_thresholds] is read during the call (the thresholds travel in the kernel arguments).
 * Per image b and threshold t, exactly EvaluateDetections.evaluate, quirks included:
 *   predictions     rows r < num_valid[b] with score[r] > S_t (strict, fp32)
 *   one_class != 0  every prediction class and every ground-truth class is taken as 0
 *   error image     a ground-truth class outside [0,nclasses): errors[t] += 1 and nothing else is counted; likewise (never from
 *                   y3_net_detect) a class outside the range among the predictions of threshold t
 *   IoU             fp32, each operation rounded on its own: ow = max(min(x2,x2') - max(x1,x1'), 0), oh likewise, inter = ow*oh,
 *                   iou = inter / ((a1 + a2) - inter); true division, no epsilon; min / max pass a NaN on
 *   best            the ground-truth row with the first maximum IoU as np.argmax takes it: a NaN (0/0 between two zero-area
 *                   boxes that do not overlap) counts as the maximum
 *   decision        iou[best] > iou_threshold && class[gt best] == class[pred]; false with no ground truth.  Every prediction
 *                   is tested against the EMPTY assignment (two predictions that pick the same ground-truth box are both TP);
 *                   `assigned` (some prediction decided for the row) only feeds fn
 *   counters        tp[c_pred] += decision, fp[c_pred] += !decision, preds[c_pred] += 1, gts[c_gt] += 1,
 *                   fn[c_gt] += !assigned, examples[t] += 1
 * counters_dev: int64 [n_thresholds][5*nclasses + 2] = preds, gts, tp, fp, fn (each [nclasses]), errors, examples.
 * ADDED to (never zeroed by) the call, so one buffer accumulates a data set; integer adds commute, the result does not depend
 * on any order.  Checked on the host before anything is enqueued (Y3_ERR_INVALID with a message): batch >= 1, max_boxes in
 * [1,1024], max_gt in [1,1024], nclasses in [1,4096], n_thresholds in [1,16], no null pointer.  The call only enqueues on
 * `stream` -- no allocation, query or synchronise -- and can be captured into a HIP graph (the thresholds are then frozen in).
 * One exception: a launch that needs more than 64 KB of LDS (20 max_gt + 20 nclasses bytes: beyond ~2000 classes) asks for the
 * current device, and the first such launch on a device raises the kernel's LDS limit once (hipFuncSetAttribute), as the conv
 * launches of y3_net_forward do.
 * Host restatement: evaluate_detections.sweep_counters.
 * ---------------------------------------------------------------------------------------- */
y3_status y3_evaluate_detections(const void *packed_dev, const int32_t *num_valid_dev, int batch, int max_boxes,
                                 const float *gt_boxes_dev /*[batch,max_gt,4]*/, const int32_t *gt_classes_dev /*[batch,max_gt]*/,
                                 const int32_t *gt_count_dev /*[batch]*/, int max_gt, int nclasses, float iou_threshold,
                                 const float *score_thresholds_host, int n_thresholds, int one_class,
                                 int64_t *counters_dev, void *stream);

/* ------------------------------------------------------------------------------------------
 * Matching for COCO-style average precision, from the same detect pass.  NO reference counterpart (the reference stops at the
 * counters above, whose quirk -- two predictions on one ground-truth box are both TP -- makes them incomparable with a published
 * mAP).  The rule is this project's statement of the COCO matching: greedy in score order, a ground-truth box matched at most once
 * per IoU threshold; no crowd flags, no area ranges, max_boxes as the per-image cap.  The tie direction is recalled from the
 * COCO evaluation's loop, not checked against pycocotools.
 * Inputs exactly as for y3_evaluate_detections: packed_dev [batch,max_boxes,7], num_valid_dev clamped to [0,max_boxes], padded
 * ground truth with counts clamped to [0,max_gt].  iou_thresholds_host [n_iou] fp32 is read during the call (the thresholds
 * travel in the kernel arguments).  Per image b:
 *   one_class != 0  every row class and every ground-truth class is taken as 0
 *   error image     a ground-truth class outside [0,nclasses), or the class of a row r < num_valid[b] outside [0,nclasses) (both
 *                   after one_class): gt_totals[nclasses] += 1 and nothing else; all its record rows are written as invalid
 *   IoU             the fp32 expression of y3_evaluate_detections, computed by the same device function
 *   matching        per threshold t_k, independently: the rows are walked in ROW ORDER r = 0 .. num_valid-1.  y3_net_detect writes
 *                   them in descending score; the call does NOT sort.  Row r may take ground-truth row g when the classes are
 *                   equal, g is not yet taken at this threshold and iou(r,g) >= t_k in fp32 (a NaN never qualifies).  Among those
 *                   it takes the largest IoU (compared as fp32 values: -0 equals +0), the HIGHER g on a tie; bit k of the row's
 *                   mask is set and g is taken at threshold k.  The masks of different thresholds are independent: a row can
 *                   match at 0.75 and not at 0.5, when a better-scored row took its box at 0.5 and fails at 0.75
 *   records         records_dev uint32 [batch][max_boxes][2]: {score bits, class | mask << 16} for r < num_valid[b] of a counted
 *                   image (the class after one_class), {0, 0xFFFFFFFF} for every other row.  EVERY row is written, the buffer may
 *                   be uninitialised; fixed slots, no cursor: the record order is a function of the input order alone
 *   gt_totals       gt_totals_dev int64 [nclasses + 2]: [c] += 1 per ground-truth row of class c, [nclasses] += 1 per error image,
 *                   [nclasses + 1] += 1 per counted image.  ADDED to, never zeroed, like counters_dev
 * Checked on the host before anything is enqueued (Y3_ERR_INVALID with a message): batch >= 1, max_boxes in [1,1024], max_gt in
 * [1,1024], nclasses in [1,4096], n_iou in [1,16], finite thresholds, no null pointer, records / gt_totals 8-byte aligned.  The
 * call only enqueues on `stream` -- no allocation, query or synchronise -- and can be captured into a HIP graph (the thresholds
 * are then frozen in).  LDS: 20 max_gt + 24 max_boxes + 4 nclasses bytes, at most 60 KB.
 * Host restatement: evaluate_detections.match_detections; the AP integral over a data set's records:
 * evaluate_detections.average_precision.
 * ---------------------------------------------------------------------------------------- */
y3_status y3_match_detections(const void *packed_dev, const int32_t *num_valid_dev, int batch, int max_boxes,
                              const float *gt_boxes_dev /*[batch,max_gt,4]*/, const int32_t *gt_classes_dev /*[batch,max_gt]*/,
                              const int32_t *gt_count_dev /*[batch]*/, int max_gt, int nclasses, const float *iou_thresholds_host,
                              int n_iou, int one_class, uint32_t *records_dev /*[batch][max_boxes][2]*/,
                              int64_t *gt_totals_dev /*[nclasses + 2]*/, void *stream);

/* ------------------------------------------------------------------------------------------
 * Validation loss from the raw head grids (reference: core/preprocess_dataset.py:19-92, _arrange_in_grid; core/loss_func.py:19-69,
 * get_loss_func; train.py:39-54, _calc_loss).  The reference picks a checkpoint by val_loss; these two calls give its four sums
 * (xy, wh, obj, class) per image and scale from the grids y3_net_forward writes.  No gradient is taken and nothing here trains;
 * the regulariser (model.losses) is not part of the result.  The Keras / TF operators are those of TF 2.8.1 / Keras 2.8.0.
 * All arithmetic is fp32 with every operation rounded on its own unless said otherwise; eps = 1e-7f, hi = 1.0f - eps,
 * sigmoid(x) = 1 / (1 + expf(-x)).
 * Ground truth as for y3_evaluate_detections: gt_boxes_dev [batch,max_gt,4] {xmin,ymin,xmax,ymax} normalised, gt_classes_dev
 * [batch,max_gt] int32, gt_count_dev [batch] clamped to [0,max_gt]; rows r < count are the reference's rows with obj = 1.
 * anchors_host [3][3][2] as for y3_yolo_decode: scale s uses anchors[s], the flattened anchor index is 3 s + a.  grid_sizes
 * [3] = g_s, each in [1,256].
 *
 * y3_yolo_assign_targets -> cells_dev [batch,max_gt] int32, bit-exact.  Per image and row r < count:
 *   best anchor   w = xmax - xmin, h = ymax - ymin; per anchor (aw, ah): inter = min(w,aw) * min(h,ah),
 *                 iou = inter / ((w*h + aw*ah) - inter), true division; best = the first maximum (anchor 0, then a later one only
 *                 when strictly greater: a NaN never wins); s = best / 3 (the reference's histogram_fixed_width_bins), a = best % 3
 *   cell          cx = (xmin + xmax) / 2, cy likewise; col = (int)(cx * (float)g_s), row = (int)(cy * (float)g_s), the cast
 *                 truncating toward zero as tf.cast does
 *   error image   a non-finite coordinate, a class outside [0,nclasses), or row / col outside [0,g_s) (the reference's scatter
 *                 raises there): the image is assigned nothing and contributes nothing to any loss term
 *   collisions    several rows on one (s,row,col,a): the highest r wins (tensor_scatter_nd_update applies updates in order)
 *   cells[b][r]   n = 3 sum_{t<s} g_t^2 + (row g_s + col) 3 + a, the row's index in decode's row order; -1 for r >= count;
 *                 -2 for a row that lost its cell; -3 for every row r < count of an error image
 *
 * y3_yolo_loss -> loss_dev double [batch][3][4], columns xy, wh, obj, class; WRITTEN, not added to.  Per image and scale s over
 * grids_dev[s] [batch,g,g,3,5+nc], t = the logits of a row, p_obj = min(max(sigmoid(t[4]), eps), hi):
 *   obj     over EVERY row of the grid (the reference has no ignore mask): -logf((1.0f - p_obj) + eps) for an unassigned row,
 *           -logf(p_obj + eps) for an assigned one (Keras' binary_crossentropy: the other product is 0 * finite)
 *   xy      over assigned rows: tw = xmax - xmin, th = ymax - ymin, scale = 2.0f - tw*th, tx = cx*(float)g - (float)col,
 *           ty = cy*(float)g - (float)row, dx = tx - sigmoid(t[0]), dy = ty - sigmoid(t[1]); term = scale * (dx*dx + dy*dy)
 *   wh      over assigned rows: lw = logf(tw / aw), lh = logf(th / ah) with the anchor of (s,a); an infinite value is replaced
 *           by 0 (tf.where(is_inf)), a NaN is not and propagates; term = scale * ((lw - t[2])^2 + (lh - t[3])^2)
 *   class   over assigned rows, sparse_categorical_crossentropy applied to probabilities: l_k = logf(min(max(sigmoid(t[5+k]),
 *           eps), hi)), m = max_k l_k, term = logf(sum_k expf(l_k - m)) - (l_c - m); exactly 0.0f with nclasses = 1
 * An image with a -3 in its cells gets twelve zeros; so does (never from y3_yolo_assign_targets with the same nclasses) an
 * image with an assigned row whose class is outside [0,nclasses).  Cells outside [0, 3 sum g_s^2) are ignored.  The cells of
 * y3_yolo_assign_targets never name one row twice within an image; if a caller's do, the row counts once, with the xy / wh /
 * class terms of the lowest r that names it.
 * The fp32 terms of one (image, scale) are summed in fp64 by ONE workgroup in an order fixed by the grid size alone: an
 * image's twelve numbers are bit-identical across runs, positions in the batch, batch sizes, max_gt and the order of its rows.
 * For a data set val_loss = sum of the 12 entries of (sum_images loss / images) -- the eager loop's loss_fn(label, output) /
 * batch_size for full batches; perGrid = its row sums, perSource[xy,wh,obj,class] = its column sums.
 *
 * Both calls check every argument on the host before anything is enqueued (Y3_ERR_INVALID with a message): batch >= 1, max_gt
 * in [1,1024], nclasses in [1,4096], grid sizes in [1,256], no null pointer, 4-byte aligned buffers (loss_dev 8-byte).  They
 * only enqueue on `stream` -- no allocation, query or synchronise -- and can be captured into a HIP graph (anchors and grid
 * sizes travel in the kernel arguments and are then frozen in).
 * Host restatements: core/preprocess_dataset.assign_targets, core/loss_func.loss_from_cells.
 * ---------------------------------------------------------------------------------------- */
y3_status y3_yolo_assign_targets(const float *gt_boxes_dev /*[batch,max_gt,4]*/, const int32_t *gt_classes_dev /*[batch,max_gt]*/,
                                 const int32_t *gt_count_dev /*[batch]*/, int batch, int max_gt, int nclasses,
                                 const int32_t grid_sizes[3], const float *anchors_host, int32_t *cells_dev /*[batch,max_gt]*/,
                                 void *stream);
y3_status y3_yolo_loss(const float *const grids_dev[3], const int32_t grid_sizes[3], int batch, int nclasses,
                       const float *anchors_host, const float *gt_boxes_dev, const int32_t *gt_classes_dev,
                       const int32_t *cells_dev, int max_gt, double *loss_dev /*[batch][3][4]*/, void *stream);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU exchange (no reference counterpart: the reference is single-device).
 * One process per GPU; images are sharded by rank and are independent end to end, so the only collective of the path
 * is the all-gather of the packed final detections (north_star: "RCCL all-gather of the final box list over xGMI").
 *   y3_comm_get_unique_id   rank 0 draws an id (Y3_COMM_ID_BYTES bytes, host) and hands it to the other ranks by any
 *                           out-of-band means (the Python host uses the torch.distributed store / broadcast)
 *   y3_comm_init_rank       every rank, on its own current device: joins the communicator (ncclCommInitRank)
 *   y3_allgather_results    packed_dev [batch,max_boxes,7] 32-bit words + num_valid_dev [batch] of this rank ->
 *                           packed_all_dev [world*batch,max_boxes,7], num_valid_all_dev [world*batch] in rank order;
 *                           equal batch on every rank; both gathers form ONE RCCL group enqueued on `stream`
 *                           (capturable into the same HIP graph as y3_net_detect).
 * ---------------------------------------------------------------------------------------- */
typedef struct y3_comm y3_comm;
#define Y3_COMM_ID_BYTES 128
y3_status y3_comm_get_unique_id(void *id_out_host);
y3_status y3_comm_init_rank(const void *id_host, int world_size, int rank, y3_comm **out);
void y3_comm_destroy(y3_comm *comm);
y3_status y3_comm_info(const y3_comm *comm, int32_t *world_size, int32_t *rank);
y3_status y3_allgather_results(y3_comm *comm, const void *packed_dev, const int32_t *num_valid_dev, int batch,
                               int max_boxes, void *packed_all_dev, int32_t *num_valid_all_dev, void *stream);

/* ------------------------------------------------------------------------------------------
 * TFRecord framing checksum (host): CRC-32C (Castagnoli) of a host buffer, unmasked.  The tfrecords input source
 * (reference: core/load_tfrecords.py:97-99, tf.data.TFRecordDataset) verifies it per record.
 * ---------------------------------------------------------------------------------------- */
uint32_t y3_crc32c(const void *data_host, size_t nbytes);

#ifdef __cplusplus
}
#endif
#endif /* Y3_H */
