// Running a planned net: one call's Forward, the Slice of it that one lane enqueues, and the entry points that run the conv program --
// forward, forward + decode, detect, the tensor read-back and the per-conv measurements.
#include <cstdlib>
#include <vector>

#include "y3_host.h"

// One call's forward: everything that belongs to the call rather than the net.  Built on the stack by each entry point that
// runs the conv program; the net itself is read-only while a forward is enqueued.
struct Forward {
    const float *images;
    float *const *grids;                     // [heads] caller's fp32 head grids
    int batch;
    hipStream_t stream;
    int lanes;                               // concurrent sub-batches this call may use (the net's y3_net_set_lanes, or 1)
    const y3::DecodeHead *heads = nullptr;   // [heads] in output order: the head convs decode their own tiles into these buffers
                                             // (per scale: first box index, grid size, anchors) instead of writing grids
    unsigned long long *clk = nullptr;       // y3_net_measure_sclk*: device buffer the stamped launch(es) write
    int clk_conv = -1;                       // ... which conv (-2: every conv, 8 words each at clk + 8 conv)
    float *ms_out = nullptr;                 // y3_net_profile_convs: milliseconds per conv slot (n_ms entries)
    int n_ms = 0;
};

// argument checks shared by the entry points that run the conv program; `heads`: the call needs detection heads
static y3_status check_forward_args(const y3_net *net, bool args_ok, int batch, bool heads, const char *who)
{
    if (!net || !args_ok || batch <= 0) return fail(Y3_ERR_INVALID, "%s: bad argument", who);
    if (heads && net->nclasses <= 0) return fail(Y3_ERR_STATE, "%s: the net was created without detection heads (nclasses = 0)", who);
    if (!net->height) return fail(Y3_ERR_STATE, "%s: call y3_net_plan first", who);
    if (batch > net->max_batch) return fail(Y3_ERR_INVALID, "%s: batch %d > planned %d", who, batch, net->max_batch);
    return Y3_OK;
}

// first image of lane l when `batch` images run on `lanes` lanes: the one split run(), y3_lane_offset and the tensor read-back share
static inline int lane_start(int batch, int lanes, int l) { return (int)((long long)batch * l / lanes); }

// The part of a forward one run() step enqueues: images [b0, b0 + nb) of the batch, as lane `lane` of `lanes`, on stream s
struct Slice {
    const y3_net *net;
    const Forward &f;
    int b0, nb, lane;
    hipStream_t s;
    int lanes;                               // the lanes this forward runs on (run(): min(f.lanes, batch))

    size_t img_elems(int t) const { return (size_t)rows(net, t) * cols(net, t) * net->tensors[t].channels; }
    // element size: head grids are always fp32; the image batch is fp32 when the Cin = 3 first-layer kernel reads it
    // (a model whose input feeds an MFMA conv directly hands bf16 in bf16 mode, fp16 in fp16 and int8 mode); everything else follows the
    // plan, per tensor (an int8 plan: fp16 before its cut, int8 behind it)
    size_t elem_bytes(int t) const
    {
        if (net->out_slot[t] >= 0) return 4;
        if (t == net->input_tensor && net->tensors[t].channels == 3) return 4;
        return net->telem[t];
    }
    size_t bytes(int t) const { return (size_t)nb * img_elems(t) * elem_bytes(t); }
    // an int8 conv's view of operand t: the int8 copy of a tensor that crosses the cut, else the tensor itself (int8 in the arena)
    bool crosses(int t) const { return t >= 0 && net->tq8[t] != nullptr; }
    void *ptr_q(int t) const { return static_cast<char *>(net->tq8[t]) + (size_t)b0 * img_elems(t); }
    // the int8 copy of tensor t for this slice's images: q = clamp(rintf((float)x * (1 / s)))
    y3_status quantize_crossing(int t) const
    {
        hipError_t e = y3::launch_quantize16_to_i8(ptr(t), ptr_q(t), (size_t)nb * img_elems(t), 1.0f / net->tscale[t], s);
        if (e != hipSuccess) return fail(Y3_ERR_HIP, "int8 copy of tensor %d: %s", t, hipGetErrorString(e));
        return Y3_OK;
    }

    void *ptr(int t) const
    {
        if (t < 0) return nullptr;
        char *base = nullptr;
        if (t == net->input_tensor) base = reinterpret_cast<char *>(const_cast<float *>(f.images));
        else if (net->out_slot[t] >= 0) base = reinterpret_cast<char *>(f.grids[net->out_slot[t]]);
        if (base) return base + (size_t)b0 * img_elems(t) * elem_bytes(t);
        // arena tensors share blocks with other (dead) tensors of different per-image size: give every lane its
        // own 1/lanes region of the block so that concurrent sub-batches never alias
        char *blk = static_cast<char *>(net->tdev[t]);
        if (!blk) return nullptr;
        if (net->dense[t]) return blk + (size_t)b0 * img_elems(t) * elem_bytes(t);
        // lane regions: y3_lane_offset (include/y3.h), 256-B aligned and disjoint; blocks carry 4 KiB of slack
        return blk + (lane ? (size_t)y3_lane_offset((long long)net->tblock[t], f.batch, lanes, lane) : 0);
    }

    // ConvArgs of conv slot `conv` in the plan's mode; a.dec set where it decodes its output in place (fused decode; its grid is then
    // not written).  The launch decision (y3::choose_conv) adds k_chunk, xcd_gn, pos_tab and border_tiles; nothing else is changed afterwards.
    y3::ConvArgs conv_args(int conv) const
    {
        const ConvSlot &c = net->convs[conv];
        const y3_conv_desc &d = c.d;
        const y3::ConvFamily &fam = y3::family_of_conv(net, conv);
        const bool i8 = y3::conv_is_i8(net, conv);
        auto rd = [&](int t) { return i8 && crosses(t) ? ptr_q(t) : ptr(t); };
        auto rd_bytes = [&](int t) { return i8 && crosses(t) ? (size_t)nb * img_elems(t) : bytes(t); };
        y3::ConvArgs a{};
        a.src0 = rd(d.src0);
        a.src1 = rd(d.src1);
        a.wpk = c.*fam.w;
        // int8: (s_in * s_w[c]) * bn_scale[c]; two-plane: the power of two its packed weights were divided by (the BN scale is folded in)
        a.scale = i8 ? c.sc_i8_dev : fam.w == &ConvSlot::wx2_dev && !c.first_layer ? c.scale_x2_dev : c.scale_dev;   // the Cin = 3 layer runs conv_first in every mode
        a.shift = c.shift_dev;
        a.residual = rd(d.residual);
        a.q_res = c.q_res;
        a.q_inv = c.q_inv;
        a.dst = ptr(d.dst);
        a.B = nb;
        a.H = net->height / d.in_div;
        a.W = net->width / d.in_div;
        a.Ho = net->height / d.out_div;
        a.Wo = net->width / d.out_div;
        a.Cin = d.cin;
        a.C0 = d.c0;
        a.Cout = d.cout;
        a.CoutPad = c.*fam.cout_pad;
        a.ksize = d.size;
        a.stride = d.stride;
        a.pad = (d.size == 3) ? 1 : 0;
        a.up0 = d.src0_upsample;
        a.leaky = d.leaky;
        a.M = nb * a.Ho * a.Wo;
        a.K = c.K;
        a.src0_bytes = (unsigned)rd_bytes(d.src0);
        a.src1_bytes = d.src1 >= 0 ? (unsigned)rd_bytes(d.src1) : 0;
        a.w_bytes = (unsigned)((size_t)a.CoutPad * c.K * fam.elem_bytes);
        a.dst_bytes = (unsigned)bytes(d.dst);
        a.n_cus = net->n_cus;
        a.device = net->device;
        a.clk_stamps = !f.clk ? nullptr : f.clk_conv == conv ? f.clk : f.clk_conv == -2 ? f.clk + 8 * conv : nullptr;   // fp32 MFMA kernel and stem only
        if (f.heads && net->out_slot[d.dst] >= 0) {
            a.dec = f.heads[net->out_slot[d.dst]];
            a.dec.boxes += (size_t)b0 * a.dec.N * 4;
            a.dec.cls += (size_t)b0 * a.dec.N;
            a.dec.scores += (size_t)b0 * a.dec.N;
            a.dst = nullptr;
            a.dst_bytes = 0;
        }
        return a;
    }

    // the fused stem launch (op 1) from conv1's own args: conv0 (op 0) and, with stem_conv2, the 1x1 of op 2 run inside it
    y3_status launch_stem(const y3::ConvArgs &a1) const
    {
        const ConvSlot &c0 = net->convs[net->ops[0].index], &c1 = net->convs[net->ops[1].index];
        const y3::ConvFamily &fam = y3::family_of_conv(net, net->ops[1].index);   // an int8 plan: the fp16 plans' stem, before the cut
        y3::StemArgs sa{};
        sa.img = static_cast<const float *>(ptr(c0.d.src0));
        sa.w0 = c0.*fam.w0_stem;
        sa.scale0 = c0.*fam.scale0_stem;
        sa.shift0 = c0.shift_dev;
        sa.w1 = c1.*fam.w;
        sa.scale1 = c1.scale_dev;
        sa.shift1 = c1.shift_dev;
        sa.dst = a1.dst;
        sa.B = nb;
        sa.H = net->height;
        sa.W = net->width;
        sa.leaky0 = c0.d.leaky;
        sa.leaky1 = c1.d.leaky;
        sa.img_bytes = (unsigned)bytes(c0.d.src0);
        sa.dst_bytes = a1.dst_bytes;
        sa.device = net->device;
        sa.n_cus = net->n_cus;
        sa.clk_stamps = a1.clk_stamps;
        if (net->stem_conv2) {
            const ConvSlot &c2 = net->convs[net->ops[2].index];
            sa.w2 = c2.*fam.w;
            sa.scale2 = c2.scale_dev;
            sa.shift2 = c2.shift_dev;
            sa.dst2 = ptr(c2.d.dst);
            sa.leaky2 = c2.d.leaky;
            sa.dst2_bytes = (unsigned)bytes(c2.d.dst);
            if (!sa.dst2) return fail(Y3_ERR_STATE, "conv %d: tensor not planned", net->ops[2].index);
        }
        hipError_t e = fam.launch_stem(sa, s);
        if (e != hipSuccess) return fail(Y3_ERR_HIP, "conv %d launch: %s", net->ops[1].index, hipGetErrorString(e));
        return Y3_OK;
    }

    // the fused tiny stem launch (op 2): conv0 (op 0), the pools of ops 1 and 3 and conv1 run inside it; it stores pool 1's tensor
    y3_status launch_tiny_stem() const
    {
        const ConvSlot &c0 = net->convs[net->ops[0].index], &c1 = net->convs[net->ops[2].index];
        const y3::ConvFamily &fam = y3::family_of_conv(net, net->ops[2].index);
        const int out = net->aux[net->ops[3].index].dst;
        y3::TinyStemArgs ta{};
        ta.img = static_cast<const float *>(ptr(c0.d.src0));
        ta.w0 = c0.w0tiny_dev;
        ta.scale0 = c0.scale_dev;
        ta.shift0 = c0.shift_dev;
        ta.w1 = c1.*fam.w1_tiny;
        ta.scale1 = c1.scale_dev;
        ta.shift1 = c1.shift_dev;
        ta.dst = ptr(out);
        ta.B = nb;
        ta.H = net->height;
        ta.W = net->width;
        ta.leaky0 = c0.d.leaky;
        ta.leaky1 = c1.d.leaky;
        ta.device = net->device;
        ta.n_cus = net->n_cus;
        if (!ta.img || !ta.dst || !ta.w0 || !ta.w1) return fail(Y3_ERR_STATE, "conv %d (fused tiny stem): tensor not planned or weights not loaded", net->ops[2].index);
        hipError_t e = fam.launch_tiny_stem(ta, s);
        if (e != hipSuccess) return fail(Y3_ERR_HIP, "conv %d (fused tiny stem) launch: %s", net->ops[2].index, hipGetErrorString(e));
        return Y3_OK;
    }

    // launch conv op oi as y3::choose_conv decided
    y3_status launch_conv(int oi, const y3::ConvArgs &a, const y3::ConvChoice &ch) const
    {
        const int conv = net->ops[oi].index;
        const ConvSlot &c = net->convs[conv];
        const y3::ConvFamily &fam = y3::family_of_conv(net, conv);
        hipError_t e;
        switch (ch.kind) {
            case y3::ConvKind::Stem: return launch_stem(a);
            case y3::ConvKind::TinyStem: return launch_tiny_stem();
            case y3::ConvKind::First: e = y3::launch_conv_first(a, static_cast<const float *>(c.w_dev), y3::dtype_of_conv(net, conv), s); break;
            case y3::ConvKind::HeadDecodeF32: e = y3::launch_conv_head_decode_f32(a, s); break;
            case y3::ConvKind::SplitK:
                if (lane >= net->split_ws_lanes) return fail(Y3_ERR_STATE, "conv %d: no split-K workspace for lane %d", conv, lane);
                e = fam.split->launch(a, ch.tile, net->out_slot[c.d.dst] >= 0, ch.split_k,
                                      static_cast<char *>(net->split_ws) + (size_t)lane * net->split_ws_lane, net->split_ws_lane, s);
                break;
            default:   // Mfma; out_f32 (bf16 / plane-split plans): the launch stores the caller's fp32 grid itself
                e = fam.launch(a, ch.tile, net->out_slot[c.d.dst] >= 0, s);
        }
        if (e != hipSuccess) return fail(Y3_ERR_HIP, "conv %d launch: %s", conv, hipGetErrorString(e));
        return Y3_OK;
    }

    y3_status run_aux(int index) const
    {
        const y3_aux_desc &x = net->aux[index];
        // an int8 plan runs an aux op on int8 tensors behind its cut (y3_net_set_pools_i8; resolve_i8 decided) and as an fp16 plan before it
        const int eb = (int)elem_bytes(x.dst);
        if (x.kind == Y3_AUX_MAXPOOL2X2_S2 || x.kind == Y3_AUX_MAXPOOL2X2_S1) {   // on the plan's stored elements: fp32, bf16, fp16 or int8 (y3_net_plan)
            const int stride = x.kind == Y3_AUX_MAXPOOL2X2_S2 ? 2 : 1;
            if (!ptr(x.src0) || !ptr(x.dst) || elem_bytes(x.src0) != elem_bytes(x.dst)) return fail(Y3_ERR_STATE, "aux op %d: tensor not planned", index);
            const int dt = eb == 4 ? (int)Y3_DTYPE_F32 : eb == 1 ? (int)Y3_DTYPE_I8 : net->dtype == Y3_DTYPE_I8 ? (int)Y3_DTYPE_F16 : net->dtype;
            hipError_t e = y3::launch_maxpool2x2(ptr(x.src0), ptr(x.dst), nb, rows(net, x.src0), cols(net, x.src0), net->tensors[x.src0].channels, stride, dt, s);
            if (e != hipSuccess) return fail(Y3_ERR_HIP, "aux op %d (max-pool) launch: %s", index, hipGetErrorString(e));
            return Y3_OK;
        }
        // The up-sample and the concat only move elements: a bf16 or fp16 plan runs them on its 16-bit tensors as on fp32 tensors of half the
        // channels (two elements per 4-byte word; YOLOv3-tiny's up-sample and its concat in front of a 3x3 conv), an int8 plan with
        // y3_net_set_pools_i8 on its int8 tensors as on fp32 tensors of a quarter of the channels, and on its fp16 tensors before the cut as an
        // fp16 plan.  The add is arithmetic and stays fp32 only, as every stand-alone op does in the plane-split plans and in an int8 plan
        // without that switch.
        const bool moves = x.kind == Y3_AUX_UPSAMPLE2X || x.kind == Y3_AUX_CONCAT;
        const bool narrow_plan = net->dtype == Y3_DTYPE_BF16 || net->dtype == Y3_DTYPE_F16 || (net->dtype == Y3_DTYPE_I8 && net->pools_i8_plan);
        const bool narrow = narrow_plan && moves && (eb == 2 || eb == 1) && eb == (net->aux_i8[index] ? 1 : 2) && (int)elem_bytes(x.src0) == eb &&
                            (x.src1 < 0 || (int)elem_bytes(x.src1) == eb);
        if (net->dtype != Y3_DTYPE_F32 && !narrow) return fail(Y3_ERR_INVALID, "stand-alone add/upsample/concat ops are fp32 only");
        auto p = [&](int t) { return static_cast<float *>(ptr(t)); };
        const int sh = rows(net, x.dst), sw = cols(net, x.dst);
        const int per = narrow ? 4 / eb : 1;   // elements per 4-byte word
        const int C = net->tensors[x.dst].channels;
        if (moves && (!p(x.src0) || !p(x.dst) || (x.kind == Y3_AUX_CONCAT && !p(x.src1)))) return fail(Y3_ERR_STATE, "aux op %d: tensor not planned", index);
        if (narrow && eb == 2 && (C % 8 || net->tensors[x.src0].channels % 8))
            return fail(Y3_ERR_INVALID, "aux op %d: a stand-alone up-sample / concat of a 16-bit plan needs channel counts that are multiples of 8", index);
        if (narrow && eb == 1 && (C % 16 || net->tensors[x.src0].channels % 16))   // y3_net_plan refused it: never reached
            return fail(Y3_ERR_INVALID, "aux op %d: a stand-alone up-sample / concat on int8 tensors needs channel counts that are multiples of 16", index);
        hipError_t e = hipSuccess;
        if (x.kind == Y3_AUX_ADD)
            e = y3::launch_add(p(x.src0), p(x.src1), p(x.dst), (size_t)nb * sh * sw * C, s);
        else if (x.kind == Y3_AUX_UPSAMPLE2X)
            e = y3::launch_upsample2x(p(x.src0), nb, sh / 2, sw / 2, C / per, p(x.dst), s);
        else if (x.kind == Y3_AUX_CONCAT)
            e = y3::launch_concat(p(x.src0), net->tensors[x.src0].channels / per, p(x.src1), net->tensors[x.src1].channels / per, (size_t)nb * sh * sw, p(x.dst), s);
        else
            return fail(Y3_ERR_INVALID, "unknown aux op kind %d", x.kind);
        if (e != hipSuccess) return fail(Y3_ERR_HIP, "aux op %d launch: %s", index, hipGetErrorString(e));
        return Y3_OK;
    }

    // Enqueue ops [op_begin, op_end) of the op list; the segment that ends the list also converts the staged outputs to fp32.
    y3_status run(int op_begin, int op_end) const
    {
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        if (f.ms_out) {
            HIP_TRY(hipEventCreate(&ev0));
            HIP_TRY(hipEventCreate(&ev1));
        }
        // int8 plans: an input handed over as fp16 that an int8 conv reads gets its int8 copy before the first op ...
        if (op_begin == 0 && crosses(net->input_tensor))
            if (y3_status st = quantize_crossing(net->input_tensor); st != Y3_OK) return st;
        for (int oi = op_begin; oi < op_end; ++oi) {
            const Op &o = net->ops[oi];
            if (o.kind != 0) {
                if (!(net->tiny_stem_fused && (oi == 1 || oi == 3)))   // (the pools inside the fused tiny stem launch run with op 2)
                    if (y3_status st = run_aux(o.index); st != Y3_OK) return st;
                // an int8 plan: a tensor an aux op writes before the cut that an int8 conv reads gets its copy behind that op (tiny: pool 3's)
                if (const int dst = net->aux[o.index].dst; crosses(dst))
                    if (y3_status st = quantize_crossing(dst); st != Y3_OK) return st;
                continue;
            }
            y3::ConvArgs a = conv_args(o.index);
            const y3::ConvChoice ch = y3::choose_conv(net, oi, a);
            // (the convs of the fused tiny stem read and write tensors that are not stored: launch_tiny_stem checks its own)
            const bool tiny = ch.kind == y3::ConvKind::TinyStem || ch.kind == y3::ConvKind::InTinyStem;
            if (!tiny && (!a.src0 || (!a.dst && !a.dec.boxes))) return fail(Y3_ERR_STATE, "conv %d: tensor not planned", o.index);
            a.k_chunk = ch.k_chunk;
            a.xcd_gn = ch.xcd_gn;
            a.pos_tab = ch.pos_tab;
            a.border_tiles = ch.border_tiles;
            if (ch.kind == y3::ConvKind::InStem || ch.kind == y3::ConvKind::InTinyStem) {   // runs inside conv1's launch (fused stem, fused tiny stem)
                if (f.ms_out && o.index < f.n_ms) f.ms_out[o.index] = 0.0f;
            } else {
                if (f.ms_out) HIP_TRY(hipEventRecord(ev0, s));
                if (y3_status st = launch_conv(oi, a, ch); st != Y3_OK) return st;
                if (f.ms_out) {
                    HIP_TRY(hipEventRecord(ev1, s));
                    HIP_TRY(hipEventSynchronize(ev1));
                    float ms = 0;
                    HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
                    if (o.index < f.n_ms) f.ms_out[o.index] = ms;
                }
            }
            // ... and a tensor written before the cut that an int8 conv reads gets its copy behind the op that wrote it
            const int dst = net->convs[o.index].d.dst;
            if (crosses(dst))
                if (y3_status st = quantize_crossing(dst); st != Y3_OK) return st;
        }
        for (int k = 0; k < net->n_heads && op_end == (int)net->ops.size(); ++k) {
            const int t = net->outputs[k];
            if (!net->staged[t]) continue;
            const size_t npix = (size_t)nb * rows(net, t) * cols(net, t);
            float *out = f.grids[k] + (size_t)b0 * img_elems(t);
            hipError_t e = net->dtype != Y3_DTYPE_I8 ? y3::launch_to_f32(net->dtype, ptr(t), out, npix, net->tensors[t].channels, s)
                           : net->telem[t] == 1      ? y3::launch_i8_to_f32(ptr(t), out, npix * net->tensors[t].channels, net->tscale[t], s)
                                                     : y3::launch_to_f32(Y3_DTYPE_F16, ptr(t), out, npix, net->tensors[t].channels, s);
            if (e != hipSuccess) return fail(Y3_ERR_HIP, "output %d conversion: %s", k, hipGetErrorString(e));
        }
        if (f.ms_out) {
            (void)hipEventDestroy(ev0);
            (void)hipEventDestroy(ev1);
        }
        return Y3_OK;
    }
};

static y3_status run(const y3_net *net, const Forward &f)
{
    if (y3_status st = check_forward_args(net, f.images && f.grids, f.batch, false, "y3_net_forward"); st != Y3_OK) return st;
    for (size_t i = 0; i < net->convs.size(); ++i)
        if (!net->convs[i].loaded) return fail(Y3_ERR_STATE, "y3_net_forward: conv %zu has no weights", i);
    if (net->dtype == Y3_DTYPE_F32X2)
        for (size_t i = 0; i < net->convs.size(); ++i)
            if (!net->convs[i].x2_ok) return fail(Y3_ERR_INVALID, "y3_net_forward: conv %zu has a weight outside the fp16 range of the two-plane mode", i);
    if (net->tiny_stem_fused && !net->convs[net->ops[0].index].tiny_pad_zero)
        return fail(Y3_ERR_INVALID, "y3_net_forward: the fused tiny stem (y3_net_set_tiny_stem_fusion) computes 16 channels of conv %d; its stored channels 16..31 "
                                    "must be zero pad channels (BN scale 0 and shift 0), and these weights give them values", net->ops[0].index);
    for (int i = 0; i < net->n_heads; ++i)
        if (!f.grids[i] || ((uintptr_t)f.grids[i] & 15)) return fail(Y3_ERR_INVALID, "y3_net_forward: grid %d null or not 16-byte aligned", i);
    if ((uintptr_t)f.images & 3) return fail(Y3_ERR_INVALID, "y3_net_forward: images not 4-byte aligned");
    Y3_ENTER_DEVICE(net);   // launches go to the net's device whatever the caller's current one is; restored on return
    const hipStream_t s = f.stream;
    const int batch = f.batch;
    // Images are independent, so the batch can run as `lanes` sub-batches on forked streams: while one sub-batch's
    // conv kernel drains (its last workgroups leave CUs under-occupied), the other sub-batch's kernel fills them.
    int lanes = f.lanes;
    while (lanes > 1 && batch / lanes < 1) --lanes;
    // where this forward leaves its images in the arena: y3_net_read_tensor gathers them from there
    net->last_batch = batch;
    net->last_lanes = lanes;
    // leading segment in chunks small enough for their activations to stay in the 256 MB Infinity Cache between the
    // conv that writes them and the one that reads them, then the rest of the op list on the whole (sub-)batch
    const int k_early = f.ms_out ? 0 : net->early_ops;
    auto run_lane = [&](int b0, int nb, hipStream_t st, int lane) -> y3_status {
        if (k_early > 0) {
            const int step = net->early_step;   // the plan's copy, >= 1 with early_ops > 0 (y3_net_plan_hw): y3_net_set_early_chunk on a planned net waits for the next plan
            for (int c0 = 0; c0 < nb; c0 += step) {
                const int cn = nb - c0 < step ? nb - c0 : step;
                y3_status r = Slice{net, f, b0 + c0, cn, lane, st, lanes}.run(0, k_early);
                if (r != Y3_OK) return r;
            }
        }
        return Slice{net, f, b0, nb, lane, st, lanes}.run(k_early, (int)net->ops.size());
    };
    if (lanes == 1) return run_lane(0, batch, s, 0);
    if (!net->fork_ev) return fail(Y3_ERR_STATE, "y3_net_forward: no lane streams (y3_net_plan creates them)");
    HIP_TRY(hipEventRecord(net->fork_ev, s));
    // equal sub-batches (measured with tools/lanes_sweep.py: weighted 2:3 / 3:4:5 splits were 2-3 % slower)
    int start[Y3_MAX_LANES + 1];
    for (int l = 0; l <= lanes; ++l) start[l] = lane_start(batch, lanes, l);
    // lane 0 runs on the caller's stream itself: its first kernel needs no cross-queue signal to start, and the join waits for the other lanes only
    // (fp32 eager step 31.324 -> 31.218 ms, +0.3 %, every round of three; bf16 graph replay unchanged: profiles/r05_ab_lane0_on_caller_stream.txt)
    hipStream_t ls[Y3_MAX_LANES];
    for (int l = 0; l < Y3_MAX_LANES; ++l) ls[l] = l == 0 ? s : net->lane_stream[l];
    for (int l = 0; l < lanes; ++l)
        if (start[l + 1] > start[l] && ls[l] != s) HIP_TRY(hipStreamWaitEvent(ls[l], net->fork_ev, 0));
    if (k_early > 0) {
        for (int l = 0; l < lanes; ++l) {
            const int nb = start[l + 1] - start[l];
            if (nb <= 0) continue;
            y3_status st = run_lane(start[l], nb, ls[l], l);
            if (st != Y3_OK) return st;
        }
    } else {
        // op-major enqueue: op k of every lane before op k+1 of any.  Enqueued lane by lane, an eager forward gives lane 0 a
        // head start of one whole forward's worth of host launch time (0.3 ms; 0.9 ms under a profiler: the per-queue timeline of
        // tools/timeline_dump.py shows lane 0 four kernels ahead), and a start offset between the lanes only costs
        // (profiles/r03_ab_lane_stagger.txt).  A captured forward replays with both branches released at once either way.
        const int n_ops = (int)net->ops.size();
        // (A start offset between the lanes was measured again in round 5 for the fp32 plan -- lane 1 released 1 / 2 / 4 ops behind lane 0: at most
        // +0.28 %, inside the process-to-process spread, profiles/r05_ab_f32_lane_stagger.txt; not kept.)
        for (int oi = 0; oi < n_ops; ++oi)
            for (int l = 0; l < lanes; ++l) {
                const int nb = start[l + 1] - start[l];
                if (nb <= 0) continue;
                y3_status st = Slice{net, f, start[l], nb, l, ls[l], lanes}.run(oi, oi + 1);
                if (st != Y3_OK) return st;
            }
    }
    for (int l = 0; l < lanes; ++l) {
        if (start[l + 1] <= start[l]) continue;
        if (ls[l] == s) continue;
        HIP_TRY(hipEventRecord(net->join_ev[l], ls[l]));
        HIP_TRY(hipStreamWaitEvent(s, net->join_ev[l], 0));
    }
    return Y3_OK;
}

extern "C" {

y3_status y3_net_forward(y3_net *net, const float *images_dev, int batch, float *const grids_dev[3], void *stream)
try {
    return run(net, {images_dev, grids_dev, batch, (hipStream_t)stream, net ? net->lanes : 1});
}
Y3_CATCH("y3_net_forward")

y3_status y3_net_profile_convs(y3_net *net, const float *images_dev, int batch, float *ms_out, int n, void *stream)
try {
    if (!net || !ms_out) return fail(Y3_ERR_INVALID, "y3_net_profile_convs: bad argument");
    // head grids go to scratch owned by this call
    if (!net->height || batch <= 0) return fail(Y3_ERR_STATE, "y3_net_profile_convs: call y3_net_plan first (and batch > 0)");
    Y3_ENTER_DEVICE(net);
    float *g[3] = {nullptr, nullptr, nullptr};
    for (int i = 0; i < net->n_heads; ++i) {
        const int t = net->outputs[i];
        hipError_t e = hipMalloc(&g[i], (size_t)batch * rows(net, t) * cols(net, t) * net->tensors[net->outputs[i]].channels * sizeof(float));
        if (e != hipSuccess) {
            for (int k = 0; k < i; ++k) (void)hipFree(g[k]);
            return fail(Y3_ERR_OOM, "y3_net_profile_convs: hipMalloc: %s", hipGetErrorString(e));
        }
    }
    Forward f{images_dev, g, batch, (hipStream_t)stream, 1};   // one lane: each launch is timed on its own
    f.ms_out = ms_out;
    f.n_ms = n;
    y3_status st = run(net, f);
    (void)hipStreamSynchronize((hipStream_t)stream);
    for (int i = 0; i < net->n_heads; ++i) (void)hipFree(g[i]);
    return st;
}
Y3_CATCH("y3_net_profile_convs")

namespace {
// can conv slot i of this plan carry the clock stamps?  The fp32 MFMA kernel (fp32 plans) and the fused stem kernel (fp32 and bf16 plans; fp16
// plans with y3_net_set_stem_fusion_f16) do.
bool conv_carries_stamps(const y3_net *net, size_t i)
{
    const int oi = y3::conv_op(net, (int)i);
    if (oi < 0) return false;
    const y3::ConvKind k = y3::choose_conv_planned(net, oi).kind;   // a split launch carries no stamps, nor does a conv inside the stem launch
    return k == y3::ConvKind::Stem || (k == y3::ConvKind::Mfma && net->dtype == Y3_DTYPE_F32);
}
// pick >= 0: that conv, *mhz_out one value; pick == -2: every conv that carries stamps, mhz_out / start_us / end_us arrays of
// convs.size() entries (0 where a conv left no stamps; times relative to the earliest stamp, from s_memrealtime)
y3_status measure_sclk_arrays(const y3_net *net, const float *images_dev, int batch, float *const grids_dev[3], int forwards,
                              int pick, float *mhz_out, double *start_us, double *end_us, void *stream)
{
    Y3_ENTER_DEVICE(net);
    const size_t nconv = net->convs.size();
    const size_t words = pick == -2 ? 8 * nconv : 8;   // per conv: memtime, realtime at entry; the same after the epilogue; realtime at the entry of workgroup 0
    std::vector<unsigned long long> host(words, 0ull);
    unsigned long long *buf = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&buf), words * sizeof(unsigned long long)));
    hipError_t e = hipMemsetAsync(buf, 0, words * sizeof(unsigned long long), (hipStream_t)stream);
    // the chip's clock follows the load of the last milliseconds: stamp the LAST of `forwards` back-to-back forwards
    y3_status st = Y3_OK;
    // one lane: one launch of a stamped conv (concurrent sub-batches would each stamp the same words)
    Forward f{images_dev, grids_dev, batch, (hipStream_t)stream, 1};
    for (int i = 0; i < forwards && st == Y3_OK && e == hipSuccess; ++i) {
        f.clk = (i == forwards - 1) ? buf : nullptr;
        f.clk_conv = (i == forwards - 1) ? pick : -1;
        st = run(net, f);
    }
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e == hipSuccess) e = hipMemcpy(host.data(), buf, words * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    (void)hipFree(buf);
    if (st != Y3_OK) return st;
    if (e != hipSuccess) return fail(Y3_ERR_HIP, "y3_net_measure_sclk: %s", hipGetErrorString(e));
    if (pick >= 0) {
        const double ticks = (double)(host[2] - host[0]), real = (double)(host[3] - host[1]);
        if (!(real > 0.0) || !(ticks > 0.0)) return fail(Y3_ERR_STATE, "y3_net_measure_sclk: conv %d left no stamps", pick);
        *mhz_out = (float)(ticks / real * 100.0);   // s_memrealtime counts at 100 MHz
        return Y3_OK;
    }
    // start = entry of the launch's FIRST workgroup (word 4; the stem kernel stamps in workgroup 0 throughout: word 1),
    // end = after the epilogue of the clock-stamped workgroup (a middle one; the stem: workgroup 0, resident to the end)
    auto first = [&](size_t c) { return host[8 * c + 4] ? host[8 * c + 4] : host[8 * c + 1]; };
    unsigned long long t0 = ~0ull;
    for (size_t c = 0; c < nconv; ++c)
        if (host[8 * c + 3] > host[8 * c + 1] && first(c) < t0) t0 = first(c);
    int stamped = 0;
    for (size_t c = 0; c < nconv; ++c) {
        const double ticks = (double)(host[8 * c + 2] - host[8 * c]), real = (double)(host[8 * c + 3] - host[8 * c + 1]);
        const bool ok = host[8 * c + 3] > host[8 * c + 1] && host[8 * c + 2] > host[8 * c];
        mhz_out[c] = ok ? (float)(ticks / real * 100.0) : 0.0f;
        if (start_us) start_us[c] = ok ? (double)(first(c) - t0) / 100.0 : 0.0;
        if (end_us) end_us[c] = ok ? (double)(host[8 * c + 3] - t0) / 100.0 : 0.0;
        stamped += ok;
    }
    if (!stamped) return fail(Y3_ERR_STATE, "y3_net_measure_sclk_all: no launch of this plan left clock stamps (fp32 plan or fused stem needed; an fp16 plan fuses its stem by y3_net_set_stem_fusion_f16)");
    return Y3_OK;
}
}  // namespace

y3_status y3_net_measure_sclk_conv(y3_net *net, const float *images_dev, int batch, float *const grids_dev[3], int forwards,
                                   int conv, float *mhz_out, void *stream)
try {
    if (!net || !mhz_out || forwards < 1 || conv < 0 || conv >= (int)net->convs.size())
        return fail(Y3_ERR_INVALID, "y3_net_measure_sclk_conv: bad argument");
    if (!conv_carries_stamps(net, (size_t)conv))
        return fail(Y3_ERR_STATE, "y3_net_measure_sclk_conv: the launch of conv %d carries no clock stamps in this plan", conv);
    return measure_sclk_arrays(net, images_dev, batch, grids_dev, forwards, conv, mhz_out, nullptr, nullptr, stream);
}
Y3_CATCH("y3_net_measure_sclk_conv")

y3_status y3_net_measure_sclk(y3_net *net, const float *images_dev, int batch, float *const grids_dev[3], int forwards,
                              float *mhz_out, void *stream)
try {
    if (!net || !mhz_out || forwards < 1) return fail(Y3_ERR_INVALID, "y3_net_measure_sclk: bad argument");
    // the launch that carries the stamps: the conv with the most FLOPs among those whose kernel has them -- the fp32 MFMA
    // kernel (fp32 plans; a steady-state workgroup of a ~0.8 ms launch) or the fused stem kernel (fp32 and bf16 plans; fp16 plans once
    // y3_net_set_stem_fusion_f16 has switched it on)
    int pick = -1;
    double best = 0;
    for (size_t i = 0; i < net->convs.size(); ++i) {
        const ConvSlot &c = net->convs[i];
        if (!conv_carries_stamps(net, i)) continue;
        const double ho = net->height / c.d.out_div, wo = net->width / c.d.out_div;   // 0 without a plan
        const double fl = 2.0 * c.d.size * c.d.size * c.d.cin * c.d.cout * ho * wo;
        if (fl > best) { best = fl; pick = (int)i; }
    }
    if (pick < 0) return fail(Y3_ERR_STATE, "y3_net_measure_sclk: no launch of this plan carries clock stamps (fp32 plan or fused stem needed; an fp16 plan fuses its stem by y3_net_set_stem_fusion_f16)");
    return measure_sclk_arrays(net, images_dev, batch, grids_dev, forwards, pick, mhz_out, nullptr, nullptr, stream);
}
Y3_CATCH("y3_net_measure_sclk")

y3_status y3_net_measure_sclk_all(y3_net *net, const float *images_dev, int batch, float *const grids_dev[3], int forwards,
                                  float *mhz_out, double *start_us, double *end_us, void *stream)
try {
    if (!net || !mhz_out || forwards < 1) return fail(Y3_ERR_INVALID, "y3_net_measure_sclk_all: bad argument");
    return measure_sclk_arrays(net, images_dev, batch, grids_dev, forwards, -2, mhz_out, start_us, end_us, stream);
}
Y3_CATCH("y3_net_measure_sclk_all")

// In how many lane regions arena tensor t of the last forward lies for a read of `batch` images (1: image i at i * image bytes).  After a
// forward on several lanes only that forward's batch can be gathered; a tensor of the chunked segment is dense whatever the lanes.
static y3_status read_lanes(const y3_net *net, int t, int batch, const char *who, int *lanes)
{
    *lanes = 1;
    if (net->dense[t] || net->last_lanes <= 1) return Y3_OK;
    // regions that follow one another without a gap (the shipped networks at a full batch): image i at i * image bytes, as after one lane
    const size_t img_bytes = (size_t)rows(net, t) * cols(net, t) * net->tensors[t].channels * net->telem[t];
    bool contiguous = true;
    for (int l = 1; l < net->last_lanes; ++l)
        contiguous = contiguous && (size_t)y3_lane_offset((long long)net->tblock[t], net->last_batch, net->last_lanes, l) ==
                                       (size_t)lane_start(net->last_batch, net->last_lanes, l) * img_bytes;
    if (contiguous) return Y3_OK;
    if (batch != net->last_batch)
        return fail(Y3_ERR_STATE, "%s: the last forward wrote %d images on %d lanes; its tensors can be read back at that batch only (asked: %d)", who,
                    net->last_batch, net->last_lanes, batch);
    *lanes = net->last_lanes;
    return Y3_OK;
}

long long y3_lane_offset(long long block_bytes, int batch, int lanes, int lane)
{
    if (block_bytes < 0 || batch < 1 || lanes < 1 || lanes > Y3_MAX_LANES || lanes > batch || lane < 0 || lane >= lanes) return -1;
    unsigned long long off = 0;
    for (int l = 1; l <= lane; ++l) {
        const unsigned long long nb = (unsigned long long)(lane_start(batch, lanes, l) - lane_start(batch, lanes, l - 1));
        const unsigned long long share = ((unsigned long long)block_bytes * nb + (unsigned long long)batch - 1) / (unsigned long long)batch;   // ceil
        off = (off + share + 255) & ~255ull;
    }
    return (long long)off;
}

y3_status y3_net_read_tensor(y3_net *net, int t, int batch, float *dst_dev, size_t *n_elems, void *stream)
try {
    if (!net || t < 0 || t >= (int)net->tensors.size() || !net->height)
        return fail(Y3_ERR_INVALID, "y3_net_read_tensor: bad argument");
    if (batch < 1 || batch > net->max_batch) return fail(Y3_ERR_INVALID, "y3_net_read_tensor: batch %d outside 1..%d of the plan", batch, net->max_batch);
    const size_t ipix = (size_t)rows(net, t) * cols(net, t);
    const size_t n = (size_t)batch * ipix * net->tensors[t].channels;
    if (n_elems) *n_elems = n;
    if (!dst_dev) return Y3_OK;
    if (net->tiny_stem_fused && net->tiny_inner[t])
        return fail(Y3_ERR_STATE, "y3_net_read_tensor: tensor %d lies inside the fused tiny stem launch and is never stored (y3_net_set_tiny_stem_fusion(net, 0) and "
                                  "a new plan keep it)", t);
    if (!net->tdev[t]) return fail(Y3_ERR_STATE, "y3_net_read_tensor: tensor %d is not held in the arena", t);
    if (net->last_batch < 1) return fail(Y3_ERR_STATE, "y3_net_read_tensor: no forward was enqueued on this plan; its arena holds nothing to read");
    int lanes = 1;
    if (y3_status st = read_lanes(net, t, batch, "y3_net_read_tensor", &lanes); st != Y3_OK) return st;
    Y3_ENTER_DEVICE(net);   // the conversion kernels / the copy below read the net's arena: enqueue them on its device
    const int C = net->tensors[t].channels;
    for (int l = 0; l < lanes; ++l) {   // one lane: the whole batch from the block start
        const int b0 = lane_start(batch, lanes, l), nb = lane_start(batch, lanes, l + 1) - b0;
        if (nb <= 0) continue;
        const char *src = static_cast<const char *>(net->tdev[t]) + (l ? (size_t)y3_lane_offset((long long)net->tblock[t], batch, lanes, l) : 0);
        float *dst = dst_dev + (size_t)b0 * ipix * C;
        const size_t npix = (size_t)nb * ipix;
        // an int8 plan: (float)q * s behind the cut, the fp16 value before it
        hipError_t e = net->dtype != Y3_DTYPE_I8 ? y3::launch_to_f32(net->dtype, src, dst, npix, C, (hipStream_t)stream)
                       : net->telem[t] == 1      ? y3::launch_i8_to_f32(src, dst, npix * C, net->tscale[t], (hipStream_t)stream)
                                                 : y3::launch_to_f32(Y3_DTYPE_F16, src, dst, npix, C, (hipStream_t)stream);
        if (e != hipSuccess) return fail(Y3_ERR_HIP, "y3_net_read_tensor: %s", hipGetErrorString(e));
    }
    return Y3_OK;
}
Y3_CATCH("y3_net_read_tensor")

y3_status y3_net_read_tensor_i8(y3_net *net, int t, int batch, int8_t *dst_dev, size_t *n_elems, void *stream)
try {
    if (!net || t < 0 || t >= (int)net->tensors.size() || !net->height || batch <= 0 || batch > net->max_batch)
        return fail(Y3_ERR_INVALID, "y3_net_read_tensor_i8: bad argument");
    const size_t img = (size_t)rows(net, t) * cols(net, t) * net->tensors[t].channels;
    const size_t n = (size_t)batch * img;
    if (n_elems) *n_elems = n;
    if (!dst_dev) return Y3_OK;
    // the int8 copy of a tensor that crosses the cut (image i at i * image bytes whatever the lanes), else an int8 tensor of the arena
    const void *src = net->dtype != Y3_DTYPE_I8 ? nullptr : net->tq8[t] ? net->tq8[t] : (net->telem[t] == 1 && net->out_slot[t] < 0) ? net->tdev[t] : nullptr;
    if (!src) return fail(Y3_ERR_STATE, "y3_net_read_tensor_i8: tensor %d is not held as int8 in this plan", t);
    if (net->last_batch < 1) return fail(Y3_ERR_STATE, "y3_net_read_tensor_i8: no forward was enqueued on this plan; its arena holds nothing to read");
    int lanes = 1;
    if (!net->tq8[t])
        if (y3_status st = read_lanes(net, t, batch, "y3_net_read_tensor_i8", &lanes); st != Y3_OK) return st;
    Y3_ENTER_DEVICE(net);
    for (int l = 0; l < lanes; ++l) {
        const int b0 = lane_start(batch, lanes, l), nb = lane_start(batch, lanes, l + 1) - b0;
        if (nb <= 0) continue;
        const char *from = static_cast<const char *>(src) + (l ? (size_t)y3_lane_offset((long long)net->tblock[t], batch, lanes, l) : 0);
        HIP_TRY(hipMemcpyAsync(dst_dev + (size_t)b0 * img, from, (size_t)nb * img, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    }
    return Y3_OK;
}
Y3_CATCH("y3_net_read_tensor_i8")

// ------------------------------------------------------------------------------------------ forward + decode
namespace {
// Can the heads decode in place?  Each output must come from a 1x1 / stride-1 single-source conv without shortcut whose
// 3 * (5 + nc) channels fit one 256-wide tile, written straight to the caller-visible grid (not staged), in an fp32, bf16
// or fp16 plan.  Y3_FUSE_DECODE=0 (tools: A/B against the composed route) switches the fusion off.
bool heads_can_decode(const y3_net *net)
{
    static const bool off = [] { const char *e = getenv("Y3_FUSE_DECODE"); return e && e[0] == '0'; }();
    if (off || net->nclasses <= 0 || (net->dtype != Y3_DTYPE_F32 && net->dtype != Y3_DTYPE_BF16 && net->dtype != Y3_DTYPE_F16 && net->dtype != Y3_DTYPE_I8)) return false;
    if (net->kept || net->early_ops > 0 || 3 * (5 + net->nclasses) > 256) return false;
    for (int k = 0; k < net->n_heads; ++k) {
        const int t = net->outputs[k];
        if (net->staged[t]) return false;
        int producers = 0;
        for (const ConvSlot &c : net->convs) {
            if (c.d.dst != t) continue;
            ++producers;
            if (c.first_layer || c.d.size != 1 || c.d.stride != 1 || c.d.src1 >= 0 || c.d.residual >= 0 || c.d.cin % 64 ||
                c.d.cout != 3 * (5 + net->nclasses) || c.cout_pad != 256)
                return false;
        }
        if (producers != 1) return false;
        // the fused route does not write the grid: nobody inside the net may read it (fp32 plans never stage an output, so a
        // consumer would read the caller's buffer -- on this route uninitialised scratch)
        for (const ConvSlot &c : net->convs)
            if (c.d.src0 == t || c.d.src1 == t || c.d.residual == t) return false;
        for (const y3_aux_desc &x : net->aux)
            if (x.dst == t || x.src0 == t || x.src1 == t) return false;
    }
    return true;
}
// The forward of `batch` images into decoded boxes / classes / scores, on the net's device, with the scratch layout L of this batch.
// grids_out: where the caller wants the raw head grids (null: nobody does, they go to the scratch if they are written at all).  The heads
// decode inside their own launch only when no grids are wanted and the graph allows it; otherwise the stand-alone decode over the grids.
y3_status forward_decode(const y3_net *net, const y3::DetectLayout &L, const float *images_dev, int batch, const float *anchors_host,
                         float *const *grids_out, float *bboxes_dev, int64_t *class_idx_dev, float *scores_dev, void *stream)
{
    char *b = static_cast<char *>(net->det_buf);
    float *scratch[3] = {reinterpret_cast<float *>(b + L.grid[0]), reinterpret_cast<float *>(b + L.grid[1]), reinterpret_cast<float *>(b + L.grid[2])};
    float *const *grids = grids_out ? grids_out : scratch;
    Forward f{images_dev, grids, batch, (hipStream_t)stream, net->lanes};
    if (grids_out || !heads_can_decode(net)) {   // composed route
        if (y3_status st = run(net, f); st != Y3_OK) return st;
        return y3::decode_scores_hw("y3_yolo_decode_scores", grids, L.gs, net->n_heads, batch, net->nclasses, anchors_host, bboxes_dev, class_idx_dev, scores_dev, stream);
    }
    y3::DecodeHead heads[3];
    int first = 0;
    for (int k = 0; k < net->n_heads; ++k) {
        heads[k].boxes = bboxes_dev;
        heads[k].cls = class_idx_dev;
        heads[k].scores = scores_dev;
        heads[k].gh = L.gs[k][0];
        heads[k].gw = L.gs[k][1];
        heads[k].off = first;
        heads[k].N = (int)L.n_boxes;
        heads[k].nc = net->nclasses;
        for (int a = 0; a < 3; ++a) {
            heads[k].anchors[a][0] = anchors_host[(k * 3 + a) * 2 + 0];
            heads[k].anchors[a][1] = anchors_host[(k * 3 + a) * 2 + 1];
        }
        first += L.gs[k][0] * L.gs[k][1] * 3;
    }
    f.heads = heads;
    return run(net, f);
}
}  // namespace

y3_status y3_net_forward_decode(y3_net *net, const float *images_dev, int batch, const float *anchors_host, float *bboxes_dev,
                                int64_t *class_idx_dev, float *scores_dev, void *stream)
try {
    y3_status st = check_forward_args(net, images_dev && anchors_host && bboxes_dev && class_idx_dev && scores_dev, batch, true,
                                      "y3_net_forward_decode");
    if (st != Y3_OK) return st;
    if ((uintptr_t)bboxes_dev & 15) return fail(Y3_ERR_INVALID, "y3_net_forward_decode: bboxes not 16-byte aligned");
    Y3_ENTER_DEVICE(net);
    const y3::DetectLayout L = y3::detect_layout(net, batch);
    if (!net->det_buf || net->det_bytes < L.total)
        return fail(Y3_ERR_STATE, "y3_net_forward_decode: detect scratch not planned (y3_net_plan allocates it)");
    return forward_decode(net, L, images_dev, batch, anchors_host, nullptr, bboxes_dev, class_idx_dev, scores_dev, stream);
}
Y3_CATCH("y3_net_forward_decode")

// ------------------------------------------------------------------------------------------ whole pipeline
// y3_net_detect (grids_out null: the raw grids are nobody's) and y3_net_detect_grids under the caller's name `who`: every check, then the
// forward with its decode -- the candidates over the grids when the net is multi-label -- then the one tail (y3::select_and_pack).
static y3_status detect(const char *who, y3_net *net, const float *images_dev, int batch, const float *anchors_host, int max_boxes,
                        float iou_threshold, float score_threshold, float *const *grids_out, void *packed_dev, int32_t *num_valid_dev, void *stream)
{
    y3_status st = check_forward_args(net, images_dev && anchors_host && packed_dev && num_valid_dev, batch, true, who);
    if (st != Y3_OK) return st;
    if (max_boxes <= 0 || max_boxes > Y3_MAX_OUTPUT_BOXES) return fail(Y3_ERR_INVALID, "%s: max_boxes must be in [1,%d]", who, Y3_MAX_OUTPUT_BOXES);
    Y3_ENTER_DEVICE(net);   // the decode / NMS / pack launches below go to the net's device; the caller's current device is restored on return
    const y3::DetectLayout L = y3::detect_layout(net, batch);
    if (!net->det_buf || net->det_bytes < L.total) return fail(Y3_ERR_STATE, "%s: detect scratch not planned (y3_net_plan allocates it)", who);
    const int n = (int)L.n_boxes;
    // Multi-label (include/y3.h, y3_net_set_multi_label): the NMS, the pack and the source rewrite run over [batch, K] candidates -- K <= n, so
    // everything lives where the n boxes would
    const int K = net->multi_label && net->multi_label_capacity ? net->multi_label_capacity : n;
    if (K > n) return fail(Y3_ERR_INVALID, "%s: multi-label capacity %d exceeds the %d boxes of the plan", who, K, n);
    if (st = y3::select_check(who, net->nms_mode, iou_threshold, score_threshold); st != Y3_OK) return st;   // before the first launch
    char *b = static_cast<char *>(net->det_buf);
    float *boxes = reinterpret_cast<float *>(b + L.boxes), *scores = reinterpret_cast<float *>(b + L.scores);
    int64_t *cls = reinterpret_cast<int64_t *>(b + L.cls);
    int32_t *sel = reinterpret_cast<int32_t *>(b + L.sel), *src = nullptr;
    if (net->multi_label) {   // the composed forward, then the candidates over its grids
        float *scratch[3] = {reinterpret_cast<float *>(b + L.grid[0]), reinterpret_cast<float *>(b + L.grid[1]), reinterpret_cast<float *>(b + L.grid[2])};
        float *const *grids = grids_out ? grids_out : scratch;
        src = reinterpret_cast<int32_t *>(b + L.cand_src);
        if (st = run(net, {images_dev, grids, batch, (hipStream_t)stream, net->lanes}); st != Y3_OK) return st;
        net->multi_label_batch = batch;
        st = y3::decode_candidates_hw(who, grids, L.gs, net->n_heads, batch, net->nclasses, anchors_host, score_threshold, K, boxes, cls, scores, src,
                                      reinterpret_cast<int32_t *>(b + L.totals), b + L.cand_ws, L.cand_ws_bytes, stream);
    } else {
        // conv program with the head convs decoding their own tiles (grids neither written nor read back) where the graph allows it.
        // (Round 5 ran NMS + pack per lane, on each lane's stream behind its last conv: bit-identical and 0.2 % slower under graph replay -- the NMS
        // workgroups take CUs from the other lane's last convs; profiles/r05_ab_bf16_lane_nms.txt.  Batch-wide launches behind the join again.)
        st = forward_decode(net, L, images_dev, batch, anchors_host, grids_out, boxes, cls, scores, stream);
    }
    if (st != Y3_OK) return st;
    return y3::select_and_pack(who, boxes, scores, cls, src, batch, K, max_boxes, net->nms_mode, iou_threshold, score_threshold, sel, num_valid_dev,
                               b + L.nms_ws, L.nms_bytes, packed_dev, stream);
}

y3_status y3_net_detect(y3_net *net, const float *images_dev, int batch, const float *anchors_host, int max_boxes,
                        float iou_threshold, float score_threshold, void *packed_dev, int32_t *num_valid_dev,
                        void *stream)
try {
    return detect("y3_net_detect", net, images_dev, batch, anchors_host, max_boxes, iou_threshold, score_threshold, nullptr, packed_dev,
                  num_valid_dev, stream);
}
Y3_CATCH("y3_net_detect")

y3_status y3_net_detect_grids(y3_net *net, const float *images_dev, int batch, const float *anchors_host, int max_boxes,
                              float iou_threshold, float score_threshold, float *const grids_out_dev[3], void *packed_dev,
                              int32_t *num_valid_dev, void *stream)
try {
    if (!grids_out_dev) return fail(Y3_ERR_INVALID, "y3_net_detect_grids: bad argument");
    return detect("y3_net_detect_grids", net, images_dev, batch, anchors_host, max_boxes, iou_threshold, score_threshold, grids_out_dev,
                  packed_dev, num_valid_dev, stream);
}
Y3_CATCH("y3_net_detect_grids")

}  // extern "C"
