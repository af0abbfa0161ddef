// Planning a net for a batch, a canvas and a mode (y3_net_plan): tensor liveness and the activation arena, the lane streams, the
// scratch of y3_net_detect, and what the planned net costs in FLOPs.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "y3_host.h"

void y3::free_plan(y3_net *n)
{
    if (n->det_buf) (void)hipFree(n->det_buf);
    n->det_buf = nullptr;
    n->det_bytes = 0;
    if (n->split_ws) (void)hipFree(n->split_ws);
    n->split_ws = nullptr;
    n->split_ws_lane = 0;
    n->split_ws_lanes = 0;
    for (const y3_net::PosTab &t : n->pos_tabs) (void)hipFree(t.dev);
    n->pos_tabs.clear();
    for (ConvSlot &c : n->convs) {
        c.pos_tab = nullptr;
        c.pos_border = 0;
    }
    for (void *p : n->blocks) (void)hipFree(p);
    n->blocks.clear();
    n->tdev.assign(n->tensors.size(), nullptr);
    n->tq8.assign(n->tensors.size(), nullptr);   // the int8 copies were blocks
}

void y3::drop_plan(y3_net *n)
{
    free_plan(n);
    n->height = n->width = n->max_batch = 0;
    n->dtype = Y3_DTYPE_F32;
    n->early_ops = n->early_step = 0;
    n->kept = 0;
    n->stem_fused = n->stem_conv2 = n->tiny_stem_fused = false;
    n->i8_first_conv = -1;
    n->aux_i8.assign(n->aux.size(), 0);
    n->pools_i8_plan = false;
    n->last_batch = n->last_lanes = 0;
    n->multi_label_batch = 0;
    for (ConvSlot &c : n->convs) c.split_k = 1;
}

// ---- border skip (fp32 3x3 convs) ---------------------------------------------------------------------------
// mask9 of output position (ho, wo): bit u * 3 + v = tap (u, v) reads input pixel (ho * stride - pad + u, wo * stride - pad + v) inside
// the H x W image -- the formula of the kernel's okmask (conv_f32.hip).  The positions go out stably sorted by mask class: by the number
// of live taps first, by mask9 among masks of equal count (a counting sort over 10 x 512 keys: positions of one mask keep their raster
// order).  A workgroup tile's positions then mostly share one mask, and the interior, one class of its own and the last, keeps the raster
// neighbourhood its L2 hits live on.  Count first because the classes meet inside tiles: in plain mask9 order a corner (4 taps) sits
// between two edge classes (6 taps) whose union with it is 8 taps -- at 52 x 52 and two positions per tile that costs 2 of 306 removable K
// tiles (304 / 12168 = 0.02498 removed against 306 / 12168 = 0.02515) -- while corners among themselves pair to 6 taps.
void y3::border_order(int Ho, int Wo, int H, int W, int stride, int pad, uint32_t *out)
{
    auto mask_of = [&](int ho, int wo) {
        uint32_t mk = 0;
        for (int u = 0; u < 3; ++u)
            for (int v = 0; v < 3; ++v) {
                const int hi = ho * stride - pad + u, wi = wo * stride - pad + v;
                if (hi >= 0 && hi < H && wi >= 0 && wi < W) mk |= 1u << (u * 3 + v);
            }
        return mk;
    };
    auto key_of = [](uint32_t mk) { return (uint32_t)__builtin_popcount(mk) * 512u + mk; };
    std::vector<int> at(10 * 512 + 1, 0);
    for (int ho = 0; ho < Ho; ++ho)
        for (int wo = 0; wo < Wo; ++wo) ++at[key_of(mask_of(ho, wo)) + 1];
    for (int k = 0; k < 10 * 512; ++k) at[k + 1] += at[k];
    for (int ho = 0; ho < Ho; ++ho)
        for (int wo = 0; wo < Wo; ++wo) {
            const uint32_t mk = mask_of(ho, wo);
            out[at[key_of(mk)]++] = pos_pack(ho, wo, mk);
        }
}

y3_status y3::resolve_border(y3_net *net)
{
    if (net->dtype != Y3_DTYPE_F32) return Y3_OK;
    for (ConvSlot &c : net->convs) {
        const y3_conv_desc &d = c.d;
        if (d.size != 3 || d.src1 >= 0 || c.first_layer) continue;
        const y3_net::PosTab g{net->height / d.out_div, net->width / d.out_div, net->height / d.in_div, net->width / d.in_div, d.stride, nullptr, 0};
        if (g.Ho > kPosMaxGrid || g.Wo > kPosMaxGrid) continue;
        for (const y3_net::PosTab &t : net->pos_tabs)
            if (t.Ho == g.Ho && t.Wo == g.Wo && t.H == g.H && t.W == g.W && t.stride == g.stride) {
                c.pos_tab = t.dev;
                c.pos_border = t.border;
            }
        if (c.pos_tab) continue;
        const size_t n = (size_t)g.Ho * g.Wo;
        std::vector<uint32_t> tab(n + kPosTabPad, 0u);   // the zero entries behind: a tile's blocks of rows >= M
        border_order(g.Ho, g.Wo, g.H, g.W, g.stride, 1, tab.data());
        net->pos_tabs.push_back(g);
        y3_net::PosTab &t = net->pos_tabs.back();   // in the list before the copy: free_plan frees it on every path
        while ((size_t)t.border < n && pos_mask(tab[t.border]) != 0x1ffu) ++t.border;   // the interior, all nine taps live, sorts last
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&t.dev), tab.size() * sizeof(uint32_t)));
        HIP_TRY(hipMemcpy(t.dev, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        c.pos_tab = t.dev;
        c.pos_border = t.border;
    }
    return Y3_OK;
}

// forked streams / events of the concurrent sub-batches: created at plan time so that a forward enqueues work only
static y3_status ensure_lanes(y3_net *net)
{
    if (net->fork_ev) return Y3_OK;
    HIP_TRY(hipEventCreateWithFlags(&net->fork_ev, hipEventDisableTiming));
    for (int i = 0; i < Y3_MAX_LANES; ++i) {
        HIP_TRY(hipStreamCreateWithFlags(&net->lane_stream[i], hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&net->join_ev[i], hipEventDisableTiming));
    }
    return Y3_OK;
}

// Arena blocks for the plan's tensors from their liveness [first, last] over the op list
static y3_status place_tensors(y3_net *net, const std::vector<int> &first, const std::vector<int> &last)
{
    const int nt = (int)net->tensors.size();
    struct Blk { void *p; size_t bytes; int free_at; };
    std::vector<Blk> pool;
    // allocate in order of first definition; the image batch and the head grids are caller-owned
    std::vector<int> order;
    for (int t = 0; t < nt; ++t) {
        const bool external = t == net->input_tensor || net->out_slot[t] >= 0;
        if (first[t] >= 0 && !external && !net->tiny_inner[t]) order.push_back(t);   // a tensor inside the fused tiny stem is never stored
    }
    std::sort(order.begin(), order.end(), [&](int a, int b) { return first[a] < first[b]; });
    for (int t : order) {
        const int until = (net->kept || net->dense[t]) ? (int)net->ops.size() + 1 : last[t];
        int pick = -1;
        for (int k = 0; k < (int)pool.size() && !net->dense[t]; ++k)
            if (pool[k].free_at < first[t] && pool[k].bytes >= net->tbytes[t] &&
                (pick < 0 || pool[k].bytes < pool[pick].bytes))
                pick = k;
        if (pick < 0) {
            void *p = nullptr;
            hipError_t e = hipMalloc(&p, net->tbytes[t] + 4096);
            if (e != hipSuccess) {
                y3::drop_plan(net);
                return fail(Y3_ERR_OOM, "y3_net_plan: hipMalloc(%zu) failed: %s", net->tbytes[t], hipGetErrorString(e));
            }
            net->blocks.push_back(p);
            pool.push_back({p, net->tbytes[t], until});
            pick = (int)pool.size() - 1;
        }
        pool[pick].free_at = until;
        net->tdev[t] = pool[pick].p;
        net->tblock[t] = pool[pick].bytes;
    }
    return Y3_OK;
}

// ---- int8 plans -------------------------------------------------------------------------------------------------------------------
// The cut c*: the first conv in op order such that it and every conv after it has Cin % 128 == 0 (both parts of a concat), and
// Cout % 16 == 0 unless it writes an fp32 grid itself.  From c* on the convs run in int8; before it the plan is an fp16 plan.  A tensor
// written before the cut (or handed in) and read behind it gets an int8 copy (tq8) from one elementwise launch.
// A conv "writes an fp32 grid itself" when its destination is a net output that a non-fp32 plan does not stage (output_staged): the one
// predicate plan_hw forms out_slot from, so the cut found before the old plan is freed is the cut the plan takes.  -> the conv count when
// no conv qualifies.
int y3::i8_cut(const y3_net *net)
{
    const int nc = (int)net->convs.size();
    int cut = nc;
    for (int i = nc - 1; i >= 0; --i) {   // conv slots are in op order
        const ConvSlot &c = net->convs[i];
        const y3_conv_desc &d = c.d;
        const bool grid = is_output(net, d.dst) && !output_staged(net, d.dst);
        const bool ok = !c.first_layer && d.cin % 128 == 0 && (d.src1 < 0 || (d.c0 % 128 == 0 && (d.cin - d.c0) % 128 == 0)) &&
                        (grid || d.cout % 16 == 0);
        if (!ok) break;
        cut = i;
    }
    return cut;
}

// Stand-alone ops of an int8 plan under y3_net_set_pools_i8 (include/y3.h, "Stand-alone ops in int8").  A tensor is behind the cut when a
// conv from the cut on or an int8 aux op writes it; walking the aux ops in op order, a pool, an up-sample or a concat runs in int8 when
// every source it has is behind the cut, and as in an fp16 plan when none is.  Reads the graph alone (no plan, no scales).
y3_status y3::resolve_i8_aux(const y3_net *net, int cut, std::vector<char> *aux_i8, std::vector<char> *behind_out)
{
    static const char *const names[] = {"add", "up-sample", "concat", "max-pool, stride 2", "max-pool, stride 1"};
    const int nt = (int)net->tensors.size(), nc = (int)net->convs.size();
    if (aux_i8) aux_i8->assign(net->aux.size(), 0);
    std::vector<char> behind(nt, 0);
    for (int i = cut; i < nc; ++i) behind[net->convs[i].d.dst] = 1;
    for (const Op &o : net->ops) {
        if (o.kind == 0 || cut >= nc || !net->pools_i8_mode) continue;
        const y3_aux_desc &x = net->aux[o.index];
        const char *name = x.kind >= 0 && x.kind <= 4 ? names[x.kind] : "unknown";
        const int n_src = x.src1 >= 0 ? 2 : 1, n_behind = behind[x.src0] + (x.src1 >= 0 ? behind[x.src1] : 0);
        if (n_behind == 0) continue;   // before the cut: the fp16 plan's op
        if (x.kind == Y3_AUX_ADD)
            return fail(Y3_ERR_INVALID, "y3_net_plan: aux op %d (%s) reads tensor %d behind the int8 cut, conv %d; a stand-alone add has no int8 form "
                                        "(a shortcut folded into its conv has)", o.index, name, behind[x.src0] ? x.src0 : x.src1, cut);
        if (n_behind < n_src)
            return fail(Y3_ERR_INVALID, "y3_net_plan: aux op %d (%s) joins tensor %d behind the int8 cut, conv %d, with tensor %d before it; both sources "
                                        "of an int8 concat must lie behind the cut", o.index, name, behind[x.src0] ? x.src0 : x.src1, cut,
                        behind[x.src0] ? x.src1 : x.src0);
        for (int t : {x.src0, x.src1})
            if (t >= 0 && is_output(net, t))
                return fail(Y3_ERR_INVALID, "y3_net_plan: aux op %d (%s) reads tensor %d, a net output behind the int8 cut (an fp32 grid, or an int8 "
                                            "tensor converted at the end of the forward); an int8 aux op reads arena tensors only", o.index, name, t);
        if (is_output(net, x.dst))
            return fail(Y3_ERR_INVALID, "y3_net_plan: aux op %d (%s) writes tensor %d, a net output; an int8 aux op writes arena tensors only", o.index, name, x.dst);
        // (no graph y3_net_create accepts gets here today: an int8 tensor is written by a conv with Cout % 16 == 0 -- the cut rule -- or moved
        // from such tensors; the guard is what the 16-byte moves rely on should the cut rule ever widen)
        for (int t : {x.src0, x.src1, x.dst})
            if (t >= 0 && net->tensors[t].channels % 16)
                return fail(Y3_ERR_INVALID, "y3_net_plan: aux op %d (%s) behind the int8 cut moves 16-byte pieces of 16 int8 channels; tensor %d has %d "
                                            "channels, no multiple of 16", o.index, name, t, net->tensors[t].channels);
        if (aux_i8) (*aux_i8)[o.index] = 1;
        behind[x.dst] = 1;
    }
    if (behind_out) *behind_out = behind;
    return Y3_OK;
}

y3_status y3::resolve_i8(y3_net *net)
{
    const int nt = (int)net->tensors.size(), nc = (int)net->convs.size();
    net->i8_first_conv = -1;
    net->telem.assign(nt, (unsigned char)conv_family(net->dtype)->elem_bytes);
    net->tq8.assign(nt, nullptr);
    net->tcross.assign(nt, 0);
    net->tscale.assign(nt, 0.0f);
    net->aux_i8.assign(net->aux.size(), 0);
    net->pools_i8_plan = net->dtype == Y3_DTYPE_I8 && net->pools_i8_mode;   // the plan's copy: the setter on a planned net waits for the next plan
    if (net->dtype != Y3_DTYPE_I8) return Y3_OK;
    const int cut = i8_cut(net);
    if (cut >= nc)
        return fail(Y3_ERR_INVALID, "y3_net_plan: no conv of this graph qualifies for int8 (the last conv needs Cin %% 128 == 0 and, unless it writes an fp32 output, Cout %% 16 == 0)");
    net->i8_first_conv = cut;
    std::fill(net->telem.begin(), net->telem.end(), (unsigned char)2);   // before the cut: an fp16 plan's tensors
    std::vector<char> behind;                                            // written by a conv behind the cut, or by an int8 aux op
    if (y3_status st = resolve_i8_aux(net, cut, &net->aux_i8, &behind); st != Y3_OK) return st;
    auto scale_of = [&](int t) { return t < (int)net->act_scale.size() && net->act_scale[t] > 0.0f ? net->act_scale[t] : 0.0f; };
    auto need = [&](int t) -> y3_status {
        if (!(scale_of(t) > 0.0f))
            return fail(Y3_ERR_STATE, "y3_net_plan: an int8 plan needs the scale of tensor %d (y3_net_set_act_scales; Net.calibrate_i8)", t);
        net->tscale[t] = scale_of(t);
        return Y3_OK;
    };
    for (int i = cut; i < nc; ++i) {
        ConvSlot &c = net->convs[i];
        const y3_conv_desc &d = c.d;
        for (int t : {d.src0, d.src1, d.residual}) {
            if (t < 0) continue;
            if (y3_status st = need(t); st != Y3_OK) return st;
            if (!behind[t]) net->tcross[t] = 1;   // its int8 copy is allocated once the arena is placed
        }
        if (d.src1 >= 0 && scale_of(d.src0) != scale_of(d.src1))
            return fail(Y3_ERR_INVALID, "y3_net_plan: conv %d concatenates tensors %d and %d with different int8 scales (%g, %g); they must be equal",
                        i, d.src0, d.src1, (double)scale_of(d.src0), (double)scale_of(d.src1));
        c.q_res = d.residual >= 0 ? scale_of(d.residual) : 0.0f;
        c.q_inv = 0.0f;
        if (net->out_slot[d.dst] < 0) {   // stores int8
            if (y3_status st = need(d.dst); st != Y3_OK) return st;
            net->telem[d.dst] = 1;
            c.q_inv = 1.0f / scale_of(d.dst);
        }
    }
    // an int8 aux op selects or moves stored bytes: its destination and every source carry one scale
    for (size_t k = 0; k < net->aux.size(); ++k) {
        if (!net->aux_i8[k]) continue;
        const y3_aux_desc &x = net->aux[k];
        if (y3_status st = need(x.dst); st != Y3_OK) return st;
        for (int t : {x.src0, x.src1}) {
            if (t < 0) continue;
            if (y3_status st = need(t); st != Y3_OK) return st;
            if (scale_of(t) != scale_of(x.dst))
                return fail(Y3_ERR_INVALID, "y3_net_plan: aux op %zu moves int8 bytes between tensors %d and %d with different int8 scales (%g, %g); they must be equal",
                            k, t, x.dst, (double)scale_of(t), (double)scale_of(x.dst));
        }
        net->telem[x.dst] = 1;
    }
    return Y3_OK;
}

y3_status y3::upload_i8_scales(y3_net *net, int slot)
{
    ConvSlot &c = net->convs[slot];
    if (!c.loaded || c.sw_host.empty()) return Y3_OK;   // follows with the weights
    const float s_in = net->tscale[c.d.src0];
    std::vector<float> sc(c.cout_pad64);
    for (int n = 0; n < c.cout_pad64; ++n) sc[n] = (s_in * c.sw_host[n]) * c.bn_scale_host[n];
    if (!c.sc_i8_dev) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c.sc_i8_dev), sc.size() * sizeof(float)));
    HIP_TRY(hipMemcpy(c.sc_i8_dev, sc.data(), sc.size() * sizeof(float), hipMemcpyHostToDevice));
    return Y3_OK;
}

y3::DetectLayout y3::detect_layout(const y3_net *net, int batch)
{
    const size_t per = (size_t)3 * (5 + net->nclasses);
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    DetectLayout L{};
    size_t n = 0, at = 0;
    for (int i = 0; i < net->n_heads; ++i) {
        L.gs[i][0] = rows(net, net->outputs[i]);
        L.gs[i][1] = cols(net, net->outputs[i]);
        L.grid[i] = at;
        at += up((size_t)batch * L.gs[i][0] * L.gs[i][1] * per * 4);
        n += (size_t)3 * L.gs[i][0] * L.gs[i][1];
    }
    L.n_boxes = n;
    L.boxes = at;
    L.cls = L.boxes + up((size_t)batch * n * 16);       // class indices (i64)
    L.scores = L.cls + up((size_t)batch * n * 8);
    L.sel = L.scores + up((size_t)batch * n * 4);       // selected indices
    L.nms_ws = L.sel + up((size_t)batch * Y3_MAX_OUTPUT_BOXES * 4);
    L.nms_bytes = nms_per_class_workspace_bytes(batch, (int)n);   // the larger of the two: the NMS mode may be switched after planning
    // always reserved: the multi-label switch may be flipped after planning as well
    L.cand_src = L.nms_ws + up(L.nms_bytes);
    L.totals = L.cand_src + up((size_t)batch * n * 4);
    L.cand_ws = L.totals + up((size_t)batch * 4);
    L.cand_ws_bytes = (size_t)batch * n * 4;
    L.total = L.cand_ws + L.cand_ws_bytes;
    return L;
}

extern "C" {

// y3_net_plan_hw's body.  freed: set once the old plan is gone -- from there on every failure, a thrown one included, ends in drop_plan
static y3_status plan_hw(y3_net *net, int max_batch, int height, int width, int dtype, bool &freed)
{
    if (!net || max_batch <= 0 || height <= 0 || width <= 0) return fail(Y3_ERR_INVALID, "y3_net_plan: bad argument");
    if (!y3::conv_family(dtype)) return fail(Y3_ERR_INVALID, "y3_net_plan: unknown dtype %d", dtype);
    if (net->has_pool && (dtype == Y3_DTYPE_F32X3 || dtype == Y3_DTYPE_F32X2 || (dtype == Y3_DTYPE_I8 && !net->pools_i8_mode)))
        return fail(Y3_ERR_INVALID, "y3_net_plan: the net holds a max-pool op (Y3_AUX_MAXPOOL2X2_*), which %s; "
                                    "Y3_DTYPE_F32, Y3_DTYPE_BF16 and Y3_DTYPE_F16 run it",
                    dtype == Y3_DTYPE_I8 ? "has no calibrated int8 form" : "does not read plane-split tensors");
    for (const y3_tensor_desc &t : net->tensors)
        if (t.div <= 0 || height % t.div || width % t.div) {
            if (height == width) return fail(Y3_ERR_INVALID, "y3_net_plan: image_size %d not divisible by %d", height, t.div);   // the square call's text, as ever
            return fail(Y3_ERR_INVALID, "y3_net_plan_hw: image size %d x %d (height x width) not divisible by %d", height, width, t.div);
        }
    if (dtype == Y3_DTYPE_F32X2)
        for (size_t i = 0; i < net->convs.size(); ++i)
            if (net->convs[i].loaded && !net->convs[i].x2_ok)
                return fail(Y3_ERR_INVALID, "y3_net_plan: conv %zu has a BN-scaled weight outside the fp16 range (|w| >= 65504); "
                                            "the two-plane mode cannot represent it, use Y3_DTYPE_F32 or Y3_DTYPE_F32X3", i);
    if (dtype == Y3_DTYPE_I8 && net->pools_i8_mode)   // what the graph itself rules out: refused with the plan in force left as it is
        if (y3_status st = y3::resolve_i8_aux(net, y3::i8_cut(net), nullptr, nullptr); st != Y3_OK) return st;
    Y3_ENTER_DEVICE(net);
    if (net->n_cus <= 0) {   // once per net: the launch path itself makes no device query
        int cus = 0;
        HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, net->device));
        net->n_cus = cus > 0 ? cus : 256;
    }
    y3::free_plan(net);
    freed = true;
    net->max_batch = max_batch;
    net->height = height;
    net->width = width;
    net->dtype = dtype;
    const int nt = (int)net->tensors.size();
    // liveness over the op list; tensors with equal lifetime class share blocks (first-fit free list)
    std::vector<int> first(nt, -1), last(nt, -1);
    auto touch = [&](int t, int i) {
        if (t < 0) return;
        if (first[t] < 0) first[t] = i;
        last[t] = i;
    };
    for (int i = 0; i < (int)net->ops.size(); ++i) {
        const Op &o = net->ops[i];
        if (o.kind == 0) {
            const y3_conv_desc &d = net->convs[o.index].d;
            touch(d.src0, i); touch(d.src1, i); touch(d.residual, i); touch(d.dst, i);
        } else {
            const y3_aux_desc &a = net->aux[o.index];
            touch(a.src0, i); touch(a.src1, i); touch(a.dst, i);
        }
    }
    // Invariant the launch path relies on: in a non-fp32 plan every output that a shortcut or first-layer conv writes is staged
    // (output_staged), so a launch that stores an fp32 grid itself (out_slot >= 0) is never a first layer and never has a residual.
    net->staged.assign(nt, 0);
    net->out_slot.assign(nt, -1);
    for (int k = net->n_heads - 1; k >= 0; --k) {   // a tensor named twice takes the first grid
        const int t = net->outputs[k];
        net->staged[t] = dtype != Y3_DTYPE_F32 && y3::output_staged(net, t);
        net->out_slot[t] = net->staged[t] ? -1 : (signed char)k;
        if (net->staged[t]) last[t] = (int)net->ops.size();          // alive until the final conversion
    }
    // chunked leading segment: every op before the (early_convs)-th conv; tensors it writes get blocks of their own,
    // laid out densely by image, because they are rewritten chunk after chunk while earlier chunks' results are still live
    // The plan keeps its own copies (kept, early_step) of the two setters it reads: y3_net_keep_activations and y3_net_set_early_chunk on a
    // planned net wait for the next plan, and nothing the planned net decides or enqueues reads their live fields
    net->kept = net->keep_all;
    net->early_ops = 0;
    net->early_step = net->early_chunk;
    if (net->early_convs > 0 && net->early_step > 0) {
        int seen = 0;
        for (int i = 0; i < (int)net->ops.size(); ++i) {
            if (net->ops[i].kind == 0 && seen++ == net->early_convs) break;
            net->early_ops = i + 1;
        }
        if (net->early_ops >= (int)net->ops.size()) net->early_ops = 0;
    }
    if (net->early_ops == 0) net->early_step = 0;   // early_ops > 0 only under the condition above: the forward's chunk loop steps by >= 1
    net->dense.assign(nt, 0);
    for (int t = 0; t < nt; ++t) net->dense[t] = (first[t] >= 0 && first[t] < net->early_ops) ? 1 : 0;
    if (y3_status st = y3::resolve_i8(net); st != Y3_OK) {   // every plan: the element size per tensor; int8 plans: the cut and the scales
        y3::drop_plan(net);
        return st;
    }
    y3::resolve_tiny_stem(net);   // before the tile check: the 32 -> 32 conv inside the fused tiny stem asks no tile table
    // A conv no tile of its mode divides (the 16-bit tables have no 32-wide tile of K step 32: y3_net_create in include/y3.h): the mode
    // cannot run the net.  Refused here, by name and before anything is allocated, not by the first forward's launch
    if (const int slot = y3::conv_without_tile(net); slot >= 0) {
        static const char *const names[] = {"fp32", "bf16", "f32x3", "f32x2", "fp16", "int8"};
        const y3_conv_desc &d = net->convs[slot].d;
        const int mode = y3::dtype_of_conv(net, slot), cut = net->i8_first_conv;
        char where[96] = "";
        if (dtype == Y3_DTYPE_I8 && mode != Y3_DTYPE_I8) snprintf(where, sizeof(where), " (it lies before the int8 cut, conv %d, and runs in fp16)", cut);
        y3::drop_plan(net);
        return fail(Y3_ERR_INVALID, "y3_net_plan: conv %d (Cin %d, c0 %d, Cout %d) has no %s tile%s: no built tile of that mode divides these "
                                    "widths (with Cin or c0 an odd multiple of 32 the 16-bit modes need Cout padded to a multiple of 64); "
                                    "Y3_DTYPE_F32, Y3_DTYPE_F32X3 and Y3_DTYPE_F32X2 run it",
                    slot, d.cin, d.src1 >= 0 ? d.c0 : -1, d.cout, names[mode], where);
    }
    for (int t = 0; t < nt; ++t) {
        net->tbytes[t] = (size_t)max_batch * rows(net, t) * cols(net, t) * net->tensors[t].channels * net->telem[t];
        // what the launches address (Slice::elem_bytes): a caller-owned fp32 grid and the fp32 image batch of the Cin = 3 layer have 4-byte
        // elements whatever the plan's format
        const bool f32 = net->out_slot[t] >= 0 || (t == net->input_tensor && net->tensors[t].channels == 3);
        const size_t addressed = f32 ? net->tbytes[t] / net->telem[t] * 4 : net->tbytes[t];
        if (addressed >= 0xFFFFFFF0ull && first[t] >= 0 && !net->tiny_inner[t]) {
            y3::drop_plan(net);
            return fail(Y3_ERR_INVALID, "y3_net_plan: tensor %d is %zu bytes; 32-bit buffer offsets need < 4 GiB, lower max_batch", t, addressed);
        }
    }
    if (y3_status st = place_tensors(net, first, last); st != Y3_OK) return st;
    net->last_batch = net->last_lanes = 0;   // no forward has written into this arena
    for (int t = 0; t < nt; ++t) {   // int8 plans: the int8 copies of the tensors that cross the cut, blocks of their own
        if (!net->tcross[t]) continue;
        const size_t bytes = (size_t)max_batch * rows(net, t) * cols(net, t) * net->tensors[t].channels;
        void *p = nullptr;
        if (hipError_t e = hipMalloc(&p, bytes + 4096); e != hipSuccess) {
            y3::drop_plan(net);
            return fail(Y3_ERR_OOM, "y3_net_plan: hipMalloc(%zu) for the int8 copy of tensor %d failed: %s", bytes, t, hipGetErrorString(e));
        }
        net->blocks.push_back(p);
        net->tq8[t] = p;
    }
    for (int i = 0; i < (int)net->convs.size(); ++i)
        if (y3::conv_is_i8(net, i))
            if (y3_status st = y3::upload_i8_scales(net, i); st != Y3_OK) {
                y3::drop_plan(net);
                return st;
            }
    if (y3_status st = ensure_lanes(net); st != Y3_OK) return st;
    {   // Y3_STEM_MODE (tools: same-process-tree A/B of the stem forms) overrides the default, not an explicit setter call
        static const int env = [] { const char *e = getenv("Y3_STEM_MODE"); return e ? atoi(e) : -1; }();
        if (env >= 0 && env <= 2 && !net->stem_mode_set) net->stem_mode = env;
    }
    y3::resolve_stem(net);
    {   // Y3_LOW_LATENCY (tools/ab_libs.py: a low-latency plan in a child process that knows nothing of it) overrides the default, not the setter
        static const int env = [] { const char *e = getenv("Y3_LOW_LATENCY"); return e ? atoi(e) : -1; }();
        if ((env == 0 || env == 1) && !net->low_latency_set) net->low_latency = env == 1;
    }
    if (net->nclasses > 0) {   // scratch of y3_net_detect: no allocation inside the stream-ordered call
        const size_t bytes = y3::detect_layout(net, max_batch).total;
        hipError_t e = hipMalloc(&net->det_buf, bytes);
        if (e != hipSuccess) {
            y3::drop_plan(net);
            return fail(Y3_ERR_OOM, "y3_net_plan: hipMalloc(%zu) for the detect scratch failed: %s", bytes, hipGetErrorString(e));
        }
        net->det_bytes = bytes;
        net->multi_label_batch = 0;   // no multi-label detect has written totals into this scratch
    }
    if (y3_status st = y3::resolve_splits(net); st != Y3_OK) {
        y3::drop_plan(net);
        return st;
    }
    if (y3_status st = y3::resolve_border(net); st != Y3_OK) {
        y3::drop_plan(net);
        return st;
    }
    return Y3_OK;
}

y3_status y3_net_plan_hw(y3_net *net, int max_batch, int height, int width, int dtype)
try {
    bool freed = false;
    y3_status st;
    try {
        st = plan_hw(net, max_batch, height, width, dtype, freed);
    } catch (...) {
        st = y3::on_exception("y3_net_plan_hw");
    }
    // (a) or (b), never a third state (include/y3.h): a failure behind free_plan -- a refusal, a HIP error, an exception -- leaves no plan
    if (st != Y3_OK && freed) y3::drop_plan(net);
    return st;
}
Y3_CATCH("y3_net_plan_hw")

void y3_border_order(int Ho, int Wo, int H, int W, int stride, int pad, uint32_t *out)
{
    if (out && Ho > 0 && Wo > 0 && Ho <= y3::kPosMaxGrid && Wo <= y3::kPosMaxGrid) y3::border_order(Ho, Wo, H, W, stride, pad, out);
}

int y3_border_tile_map(int T, int Tb, int gm, int tilesN, int32_t *out)
{
    if (T < 1 || Tb < 0 || Tb > T || (gm != 1 && gm != 2 && gm != 4 && gm != 8) || tilesN < 1 || tilesN % (8 / gm)) return -1;
    const int gn = 8 / gm, grid = y3::balanced_grid(gn, tilesN, Tb, T);
    for (int bid = 0; out && bid < grid; ++bid) {
        const y3::TileMN t = y3::balanced_tile(bid, gn, tilesN, Tb, T);
        out[2 * bid] = t.mt;
        out[2 * bid + 1] = t.mt < 0 ? -1 : t.nt;
    }
    return grid;
}

y3_status y3_net_plan(y3_net *net, int max_batch, int image_size, int dtype)
try {
    return y3_net_plan_hw(net, max_batch, image_size, image_size, dtype);
}
Y3_CATCH("y3_net_plan")

int y3_net_get_plan(const y3_net *net, int *max_batch, int *height, int *width, int *dtype)
{
    const bool planned = net && net->height > 0;
    if (max_batch) *max_batch = planned ? net->max_batch : 0;
    if (height) *height = planned ? net->height : 0;
    if (width) *width = planned ? net->width : 0;
    if (dtype) *dtype = planned ? net->dtype : (int)Y3_DTYPE_F32;
    return planned ? 1 : 0;
}

int y3_net_get_early_chunk(const y3_net *net, int *chunk_images)
{
    const bool planned = net && net->height > 0;
    if (chunk_images) *chunk_images = planned ? net->early_step : 0;
    return planned ? net->early_ops : 0;
}

double y3_net_flops_per_image(const y3_net *net)
{
    if (!net || !net->height) return 0.0;
    double tot = 0;
    for (const ConvSlot &c : net->convs) {
        const double ho = net->height / c.d.out_div, wo = net->width / c.d.out_div;
        tot += 2.0 * c.d.size * c.d.size * c.d.cin * c.d.cout * ho * wo;
    }
    return tot;
}

}  // extern "C"
