// Model handle, weight loading / BN folding / repacking, workspace arena and the forward
// pass orchestration of libvltk_hip.so.
//
// Replaces (reference vltk/modeling/frcnn.py): FRCNN.__init__ :1744-1755, build_backbone
// :200-261, Res5ROIHeads.__init__ :1312-1363, the local branch of from_pretrained's
// load_state_dict :1862-1881, and FRCNN.inference :1942-2004 (call order of backbone ->
// proposal generator -> roi heads -> roi outputs).
//
// Data layout in HBM: every activation is NHWC in the handle's precision; one arena
// (single hipMalloc, re-grown only when a larger problem arrives) holds all intermediates
// so the steady state allocates nothing; a second one serves forwards that overlap (fwd_route).  The Res5 head runs over RoI *chunks* so that the
// chunk's intermediates (pooled 14x14x1024 -> ... -> 14x14x2048) stay resident in the
// 256 MiB Infinity Cache between consecutive convolutions instead of round-tripping HBM.
#include <climits>
#include <cmath>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "vk_common.h"

namespace vk {

struct HostTensor {
    std::vector<int64_t> shape;
    std::vector<float> data;
    bool loaded = false;
};

struct ConvLayer {
    std::string prefix;
    int cin = 0, cout = 0, k = 1, stride = 1, pad = 0, dil = 1;
    bool bn = true, relu = false;
    void *w = nullptr;       // device, packed
    float *b = nullptr;      // device, [packed_cout]
    int groups = 1;          // conv2 of a ResNeXt bottleneck (frcnn.py:950)
    int dt = -1;             // storage / arithmetic type of this layer; -1: the model's (vk_handle::dt)
};

struct Block {
    ConvLayer conv1, conv2, conv3, shortcut;
    bool has_shortcut = false;
    // fp16 fast mode: conv3 and a stride-1 projection shortcut run as ONE GEMM over K = [conv3 input | block
    // input] (`out += shortcut`, frcnn.py:970-977, without storing the shortcut): conv3.w / conv3.b then hold
    // the concatenated rows and the summed bias, and shortcut.w stays null
    bool fused_shortcut = false;
};

static const int kBlocks[3][4] = {{3, 4, 6, 3}, {3, 4, 23, 3}, {3, 8, 36, 3}};   // frcnn.py:226

}  // namespace vk

using namespace vk;

struct vk_handle {
    vk_config cfg;
    int device = 0;
    vk_dtype dt = VK_F16;
    // the box predictor (three small GEMMs + the box-delta rows, frcnn.py:1726-1740) runs in fp32 in BOTH modes: its
    // inputs are the fp32 RoI features, and fp16 weights / inputs alone would put the class and attribute logits at
    // 1.1e-3 / 2.0e-3 of the fp32 reference (measured) where north_star asks 1e-3; costs ~1 ms per 9600 RoIs
    vk_dtype pdt = VK_F32;
    bool finalized = false;
    std::vector<std::string> names;                 // expected state-dict tensors (strict load)
    std::map<std::string, HostTensor> host;

    ConvLayer stem;
    std::vector<Block> stages[3];                   // res2, res3, res4
    std::vector<Block> res5;
    ConvLayer rpn_conv, rpn_heads;                  // rpn_heads = [objectness | anchor_deltas] fused 1x1
    ConvLayer cls_score, fc_attr, attr_score;       // plain GEMMs (1x1 "convs" over K RoIs)
    void *bbox_w = nullptr;                         // [4C][F] in pdt (the predictor's precision), unpadded rows (gathered per RoI)
    float *bbox_b = nullptr;
    void *emb = nullptr;                            // [C+1][F/8] in dt
    float *cell_anchors = nullptr;                  // [A][4]
    int A = 0, res4_c = 0, res5_c = 0, hid = 0, emb_dim = 0;
    std::vector<void *> owned;                      // device allocations to free

    // Everything a forward writes between fwd_open and fwd_close, twice (option forward_lanes = 2): ticket t works in
    // sets[t & 1] on lanes[t & 1], so that consecutive forwards run beside each other on the device.  The second set is
    // taken the first time a forward begins while another is open; until then (and with one lane) every forward uses
    // sets[0] on the caller's stream.
    struct WorkSet {
        char *arena = nullptr;
        size_t arena_bytes = 0;
        // per-class selection (vk_forward_begin_select): its scores / all-class deltas / confidences live apart from the arena,
        // so that the class-max mode never pays for them; taken on the first per-class forward, grown on need
        char *pc_arena = nullptr;
        size_t pc_arena_bytes = 0;
        // selection = "detections": its scores / deltas / candidate and survivor lists, a third allocation on the same terms
        char *det_arena = nullptr;
        size_t det_arena_bytes = 0;
    } sets[2];
    struct Lane {
        hipStream_t main = nullptr;                  // the lane's own stream (two-set mode only)
        hipEvent_t ev_fork = nullptr, ev_join = nullptr;
        hipEvent_t more_joins[2] = {nullptr, nullptr};
    } lanes[2];
    int forward_lanes = 0;                           // 1 = every forward on the caller's stream
    bool two_sets = false;                           // forwards have overlapped: tickets alternate between the sets from now on
    bool two_sets_failed = false;                    // the second arena could not be allocated: one set for the rest of the handle's life
    int64_t lane_forwards = 0;                       // forwards that were enqueued on a lane's stream (vk_get_option "lane_forwards")
    int cur_set = 0;                                 // the set / caller's stream of the forward being enqueued (fwd_open .. fwd_close)
    hipStream_t cur_caller = nullptr;
    const void *bbox_lin_w = nullptr;               // bbox_pred as the linear path reads it: rows padded to whole 128-row tiles
    const float *bbox_lin_b = nullptr;              // (bbox_w / bbox_b themselves when 4C is already a multiple of 128)
    // the writable options (kOptions below has their keys, defaults and ranges; vk_create sets them)
    int head_chunk = 0;                             // RoIs per Res5 chunk, 0 = all at once
    int backbone_streams = 0;                       // 2: res3/res4 as two half-batches on two streams
    int backbone_split_min_batch = 0;               // ... from this batch size on
    int head_streams = 0;                           // 2: each Res5 chunk as two half-chunks on two streams
    int head_split_min_rois = 0;                    // ... for chunks of at least this many RoIs
    int head_dedupe = 0;                            // 1: Res5 block 0 pools and convolves each distinct RoIPool window once
    int head_dedupe_taps = 0;                       // 1: ... and its 1x1 GEMMs, with conv1 of block 1, run once per distinct nine-window neighbourhood
    // the box pooler (vk_set_pooler; not an option: it changes the results): VK_POOLER_*, and RoIAlign's samples per bin and axis
    int pooler_type = VK_POOLER_ROIPOOL, pooler_sampling_ratio = 0;
    int64_t dedupe_chunks = 0;                                            // head chunks that took that path (vk_get_option "dedupe_chunks")
    int64_t indexed_chunks = 0;                                           // those of them whose conv2 read conv1's rows through the index ("indexed_chunks")
    int64_t tap_dedupe_chunks = 0;                                        // those of them that went on over the distinct neighbourhoods ("tap_dedupe_chunks")
    int64_t out_indexed_chunks = 0;                                       // those of these whose conv2 of block 0 stored the distinct rows itself ("out_indexed_chunks")
    // "pooled" after a forward whose one chunk took the dedupe path: the dense tensor was never written; vk_get_stage expands
    // src[idx] into the plan's buffer the first time the stage is asked for
    struct {
        bool pending = false;
        const void *src = nullptr;
        const int32_t *idx = nullptr;
        long rows = 0;
        int row_bytes = 0;
        void *dst = nullptr;
    } pooled_expand;

    // stage bookkeeping of the last forward
    struct Stage {
        const void *ptr;
        vk_dtype dt;
        int64_t shape[4];
        int ndim;
    };
    std::map<std::string, Stage> stages_out;
    KernelTimer *ktimer = nullptr;
    bool timing = false;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    // second stream of the res4 stage (half-batch pipelining), third / fourth when backbone_streams is 3 / 4.  Both lanes
    // fork onto the same side streams (the fork / join events are the lane's): a process stays within four streams
    hipStream_t side = nullptr;
    hipStream_t more_sides[2] = {nullptr, nullptr};
    bool ev_valid = false;
    // forwards in flight (vk_forward_begin .. vk_forward_end): ticket t uses slot t % VK_MAX_INFLIGHT
    static constexpr int VK_MAX_INFLIGHT = 4;
    int32_t *flag_host = nullptr;                   // pinned [VK_MAX_INFLIGHT]: the non-finite flag of each forward
    char *meta_host = nullptr;                      // pinned [VK_MAX_INFLIGHT][meta_cap]: image_hw + scales_yx of each forward
    size_t meta_cap = 0;
    hipEvent_t ev_done[VK_MAX_INFLIGHT] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_in[VK_MAX_INFLIGHT] = {nullptr, nullptr, nullptr, nullptr};        // the caller's stream at _begin (inputs ready)
    hipStream_t slot_stream[VK_MAX_INFLIGHT] = {nullptr, nullptr, nullptr, nullptr}; // where the ticket's forward was enqueued
    hipStream_t slot_caller[VK_MAX_INFLIGHT] = {nullptr, nullptr, nullptr, nullptr}; // the stream its caller passed
    int slot_set[VK_MAX_INFLIGHT] = {-1, -1, -1, -1};                                // its working set (-1: it launched nothing)
    int64_t next_ticket = 0, oldest_open = 0;       // tickets [oldest_open, next_ticket) have not been ended
};

// The writable options (vk_set_option / vk_get_option), one row each: vk_option_check, vk_option_default, vk_set_option,
// vk_get_option and vk_create all loop over this table.  A value is legal in [lo, hi].  `env` names the VK_* variable that
// vk_option_default puts over the built-in default, read by one of three rules.
enum EnvRule {
    ENV_NONE,
    ENV_ATOI_POSITIVE,      // atoi of the text where that is > 0 (a 0 is set with vk_set_option only)
    ENV_FIRST_DIGIT,        // the first character, where it is a digit in [lo, hi]
    ENV_ONE_DIGIT,          // the same, and nothing may follow it: anything else is ignored
};
static constexpr struct OptionRow {
    const char *key;
    int vk_handle::*member;
    int def, lo, hi;
    const char *range_msg;
    const char *env;
    EnvRule rule;
} kOptions[] = {
    {"head_chunk", &vk_handle::head_chunk, 9600, 0, INT_MAX, "head_chunk must be >= 0 (0 = all RoIs at once)", "VK_HEAD_CHUNK", ENV_ATOI_POSITIVE},
    {"backbone_streams", &vk_handle::backbone_streams, 2, 1, 4, "backbone_streams must be 1..4", "VK_BACKBONE_STREAMS", ENV_FIRST_DIGIT},
    {"head_streams", &vk_handle::head_streams, 1, 1, 2, "head_streams must be 1 or 2", "VK_HEAD_STREAMS", ENV_FIRST_DIGIT},
    {"forward_lanes", &vk_handle::forward_lanes, 2, 1, 2, "forward_lanes must be 1 or 2", "VK_FORWARD_LANES", ENV_ONE_DIGIT},
    {"head_dedupe", &vk_handle::head_dedupe, 1, 0, 1, "head_dedupe must be 0 or 1", "VK_HEAD_DEDUPE", ENV_ONE_DIGIT},
    {"head_dedupe_taps", &vk_handle::head_dedupe_taps, 1, 0, 1, "head_dedupe_taps must be 0 or 1", nullptr, ENV_ONE_DIGIT},   // (variable: vk_option_default)
    {"head_split_min_rois", &vk_handle::head_split_min_rois, 512, 2, INT_MAX, "head_split_min_rois must be >= 2", nullptr, ENV_NONE},
    {"backbone_split_min_batch", &vk_handle::backbone_split_min_batch, 8, 2, INT_MAX, "backbone_split_min_batch must be >= 2", nullptr, ENV_NONE},
};

static const OptionRow *find_option(const char *key) {
    for (const OptionRow &o : kOptions)
        if (!strcmp(key, o.key)) return &o;
    set_error("unknown option '%s'", key);
    return nullptr;
}

namespace vk {

static void add_conv_names(std::vector<std::string> &n, const std::string &p, bool bn) {
    n.push_back(p + ".weight");
    if (bn) {
        n.push_back(p + ".norm.weight");
        n.push_back(p + ".norm.bias");
        n.push_back(p + ".norm.running_mean");
        n.push_back(p + ".norm.running_var");
    } else {
        n.push_back(p + ".bias");
    }
}

static Block make_block(const std::string &p, int cin, int cmid, int cout, int stride, int dil, bool stride_in_1x1,
                        int groups, std::vector<std::string> &names) {
    Block b;
    const int s1 = stride_in_1x1 ? stride : 1, s3 = stride_in_1x1 ? 1 : stride;   // frcnn.py:932
    b.has_shortcut = cin != cout;
    if (b.has_shortcut) {
        b.shortcut = ConvLayer{p + ".shortcut", cin, cout, 1, stride, 0, 1, true, false};
        add_conv_names(names, b.shortcut.prefix, true);
    }
    b.conv1 = ConvLayer{p + ".conv1", cin, cmid, 1, s1, 0, 1, true, true};
    b.conv2 = ConvLayer{p + ".conv2", cmid, cmid, 3, s3, dil, dil, true, true};
    b.conv2.groups = groups;                                                        // frcnn.py:950
    b.conv3 = ConvLayer{p + ".conv3", cmid, cout, 1, 1, 0, 1, true, true};   // relu after the residual add
    add_conv_names(names, b.conv1.prefix, true);
    add_conv_names(names, b.conv2.prefix, true);
    add_conv_names(names, b.conv3.prefix, true);
    return b;
}

static int dev_alloc(vk_handle *h, size_t bytes, void **out) {
    void *p = nullptr;
    VK_CHECK_HIP(hipMalloc(&p, bytes ? bytes : 16));
    h->owned.push_back(p);
    *out = p;
    return VK_OK;
}

static int upload(vk_handle *h, const void *host, size_t bytes, void **out) {
    VK_TRY(dev_alloc(h, bytes, out));
    VK_CHECK_HIP(hipMemcpy(*out, host, bytes, hipMemcpyHostToDevice));
    return VK_OK;
}

static const HostTensor *get_t(vk_handle *h, const std::string &name, std::vector<int64_t> shape) {
    auto it = h->host.find(name);
    if (it == h->host.end() || !it->second.loaded) {
        set_error("missing weight '%s' (strict load)", name.c_str());
        return nullptr;
    }
    if (it->second.shape != shape) {
        std::string got, want;
        for (auto v : it->second.shape) got += std::to_string(v) + ",";
        for (auto v : shape) want += std::to_string(v) + ",";
        set_error("weight '%s' has shape [%s], expected [%s]", name.c_str(), got.c_str(), want.c_str());
        return nullptr;
    }
    return &it->second;
}

// The four BatchNorm tensors of the conv at `prefix`, one after the other: [weight | bias | running_mean | running_var] x cout
static int gather_bn(vk_handle *h, const std::string &prefix, int cout, std::vector<float> &bn) {
    const char *parts[4] = {".norm.weight", ".norm.bias", ".norm.running_mean", ".norm.running_var"};
    bn.resize(4 * (size_t)cout);
    for (int i = 0; i < 4; ++i) {
        const HostTensor *t = get_t(h, prefix + parts[i], {cout});
        if (!t) return VK_EWEIGHTS;
        memcpy(bn.data() + (size_t)i * cout, t->data.data(), sizeof(float) * cout);
    }
    return VK_OK;
}

// Packed rows (BN folded, or with the layer's plain bias) + bias of one conv on the host, in the layer's precision
static int pack_conv_host(vk_handle *h, const ConvLayer &L, std::vector<char> &packed, std::vector<float> &pb) {
    const HostTensor *w = get_t(h, L.prefix + ".weight", {L.cout, L.cin / L.groups, L.k, L.k});
    if (!w) return VK_EWEIGHTS;
    std::vector<float> bn;
    const float *bias = nullptr;
    if (L.bn) {
        VK_TRY(gather_bn(h, L.prefix, L.cout, bn));
    } else {
        const HostTensor *t = get_t(h, L.prefix + ".bias", {L.cout});
        if (!t) return VK_EWEIGHTS;
        bias = t->data.data();
    }
    const vk_dtype ldt = L.dt >= 0 ? (vk_dtype)L.dt : h->dt;
    packed.resize(vk_packed_weight_bytes(L.cout, L.cin, L.k, L.k, L.groups, ldt));
    pb.resize(vk_packed_cout(L.cout));
    return vk_pack_conv_weight(w->data.data(), L.bn ? bn.data() : nullptr, bias, L.cout, L.cin, L.k, L.k, L.groups, ldt, packed.data(), pb.data());
}

static int finalize_conv(vk_handle *h, ConvLayer &L) {
    std::vector<char> packed;
    std::vector<float> pb;
    VK_TRY(pack_conv_host(h, L, packed, pb));
    VK_TRY(upload(h, packed.data(), packed.size(), &L.w));
    return upload(h, pb.data(), pb.size() * sizeof(float), (void **)&L.b);
}

static int finalize_block(vk_handle *h, Block &b) {
    VK_TRY(finalize_conv(h, b.conv1));
    VK_TRY(finalize_conv(h, b.conv2));
    b.fused_shortcut = b.has_shortcut && vk_fuse_shortcut(b.conv3.cin, b.shortcut.cin, b.conv3.cout, b.shortcut.stride, h->dt);
    if (!b.fused_shortcut) {
        if (b.has_shortcut) VK_TRY(finalize_conv(h, b.shortcut));
        return finalize_conv(h, b.conv3);
    }
    std::vector<char> w3, wsc;
    std::vector<float> b3, bsc;
    VK_TRY(pack_conv_host(h, b.conv3, w3, b3));
    VK_TRY(pack_conv_host(h, b.shortcut, wsc, bsc));
    const size_t r3 = (size_t)b.conv3.cin * 2, rsc = (size_t)b.shortcut.cin * 2, rows = b3.size();
    std::vector<char> cat(rows * (r3 + rsc));
    for (size_t r = 0; r < rows; ++r) {
        memcpy(cat.data() + r * (r3 + rsc), w3.data() + r * r3, r3);
        memcpy(cat.data() + r * (r3 + rsc) + r3, wsc.data() + r * rsc, rsc);
        b3[r] += bsc[r];
    }
    VK_TRY(upload(h, cat.data(), cat.size(), &b.conv3.w));
    VK_TRY(upload(h, b3.data(), b3.size() * sizeof(float), (void **)&b.conv3.b));
    return VK_OK;
}

// ---- arena ----
// fp16 fast mode: `box_features.mean(dim=[2,3])` (frcnn.py:1401) is folded into the last Res5 conv3's epilogue when
// a 128-row tile cannot span more than two RoIs (14x14 maps; RES5HALVE's 7x7 maps take the separate kernel)
// `rows`: pixels of one Res5 chunk.  The kernels of the fused form address the conv3 input with 32-bit byte offsets
// (conv_duo_pool_ok): a chunk whose [rows x mid channels] f16 tensor reaches 4 GiB (ResNeXt-152 32x8d at 9600 RoIs: 7.7 GB)
// keeps the separate mean kernel instead of failing the forward.
static bool fused_mean_ok(const vk_handle *h, int P, size_t rows) {
    static const bool off = env_set("VK_NO_FUSED_MEAN");
    const long mid5 = (long)h->cfg.num_groups * h->cfg.width_per_group * 8;
    return !off && h->dt == VK_F16 && h->cfg.res5_halve == 0 && P * P >= 128 && P * P <= 255 && h->res5_c % 256 == 0 &&
           (long)rows * mid5 * 2 < (1L << 32);
}

// What does not depend on a chunk's size in the decision for the dedupe path of Res5 block 0 (fwd_head has the rest: the two GEMMs'
// routes): the plan carves the table's buffers on this.
static bool head_dedupe_planned(const vk_handle *h) {
    if (h->pooler_type != VK_POOLER_ROIPOOL) return false;     // distinct RoIPool windows mean nothing to RoIAlign
    if (!h->head_dedupe || h->dt != VK_F16 || h->cfg.res5_halve != 0 || h->head_streams != 1 || h->res5.size() < 2) return false;
    const Block &b = h->res5[0];
    for (size_t i = 1; i < h->res5.size(); ++i)          // (h_sc holds the distinct pooled rows until the forward ends)
        if (h->res5[i].has_shortcut && !h->res5[i].fused_shortcut) return false;
    return b.fused_shortcut && b.conv1.stride == 1 && b.conv2.stride == 1 && b.conv3.cin % 128 == 0 && b.conv3.cin >= 256 && b.conv2.cout == b.conv3.cin;
}

struct Carver {
    char *base;
    size_t off = 0;
    explicit Carver(char *b) : base(b) {}
    void *take(size_t bytes) {
        void *p = base ? base + off : nullptr;
        off += align_up(bytes ? bytes : 16, 256);
        return p;
    }
};

struct Plan {
    // geometry
    int N, H, W, Hp, Wp, H1, W1, Hs[3], Ws[3], Hf, Wf, R, K, P, chunk;
    // buffers
    void *img_pad, *stem_out, *bufA, *bufB, *bufSC, *bufT1, *bufT2;
    void *rpn_hid;
    float *rpn_out, *prop_boxes, *prop_logits, *rois;
    int32_t *prop_counts, *image_hw, *nonfinite;
    float *scales;
    void *bands;             // ignorey: [N][<= VK_MAX_IGNOREY][2] f32 or f64, as the ticket's slot holds them
    int32_t *band_counts;    // [N]
    void *rpn_ws;
    size_t rpn_ws_bytes;
    void *pooled, *h_t1, *h_t2, *h_a, *h_b, *h_sc;
    // the dedupe path of Res5 block 0 (fwd_head), or null: idx [chunk rows], win [chunk rows][5], one window count per chunk, the
    // table's workspace.  The distinct pooled rows live in h_sc (unused where the shortcut is fused) and conv1's distinct rows in
    // h_t2 (dead until conv2 writes it), or in h_t1 where conv2 reads them through the index (head_block0_dedupe), each large enough
    // for a chunk without a single repeated window.
    int32_t *dd_idx, *dd_win, *dd_u;
    void *dd_ws;
    size_t dd_ws_bytes;
    // ... over the distinct nine-window neighbourhoods (head_dedupe_taps), or null: nid [chunk rows], rep and idx_rep
    // [chunk rows] (a chunk without one repeated neighbourhood fits), one neighbourhood count per chunk, the table's workspace;
    // out_row [chunk rows]: where conv2 of block 0 stores each dense row among the distinct ones, -1 = nowhere
    int32_t *nb_nid, *nb_rep, *nb_idx_rep, *nb_v, *nb_out_row;
    void *nb_ws;
    size_t nb_ws_bytes;
    size_t head_rows;        // pixels that h_t1 .. h_sc hold each (a Res5 chunk, or the whole res4 map of a grid forward)
    float *pool_part;        // per-tile column sums of the last Res5 conv3 (fused spatial mean), or nullptr
    float *feat;
    void *featT, *concat, *attr_hid;
    float *cls_logits, *attr_logits, *obj_prob, *attr_prob, *chosen;
    int32_t *obj_cls, *attr_cls, *max_class;
    int64_t *keep_ids;
    size_t total;
};

// R: RoI rows per image (POST_NMS_TOPK_TEST for detection, B for given boxes, Gh * Gw for a grid); D: the output width of
// keep_ids.  whole_map (grid forward): Res5 runs over the res4 map itself, so the head buffers hold at least N * Hf * Wf
// pixels -- with R = Gh * Gw alone a 1 x 1 grid would get 196 rows per image for a map of thousands.
static Plan make_plan(vk_handle *h, char *base, int N, int H, int W, int D, int R, bool whole_map = false) {
    Plan p;
    memset(&p, 0, sizeof(p));
    const vk_config &c = h->cfg;
    const size_t es = dtype_size(h->dt);
    p.N = N;
    p.H = H;
    p.W = W;
    conv_out_hw(H, W, 7, 2, 3, 1, &p.H1, &p.W1);
    p.Hp = std::max(H + 6, 2 * p.H1 + 6);
    p.Wp = std::max(W + 6, 2 * p.W1 + 6);
    p.Wp = (p.Wp + 1) & ~1;
    int h2, w2;
    vk_stem_out_hw(H, W, c.caffe_maxpool, &h2, &w2);
    p.Hs[0] = h2;
    p.Ws[0] = w2;
    for (int s = 1; s < 3; ++s) conv_out_hw(p.Hs[s - 1], p.Ws[s - 1], 1, 2, 0, 1, &p.Hs[s], &p.Ws[s]);
    p.Hf = p.Hs[2];
    p.Wf = p.Ws[2];
    p.R = R;
    p.K = N * p.R;
    p.P = c.pooler_resolution;
    p.chunk = std::min(h->head_chunk > 0 ? h->head_chunk : p.K, p.K);

    Carver cv(base);
    p.img_pad = cv.take((size_t)N * p.Hp * p.Wp * 4 * es);
    p.stem_out = cv.take((size_t)N * p.H1 * p.W1 * c.stem_out_channels * es);
    size_t max_out = 0, max_mid = 0;
    int cout = c.res2_out_channels, cmid = c.num_groups * c.width_per_group;
    for (int s = 0; s < 3; ++s) {
        const size_t px_out = (size_t)N * p.Hs[s] * p.Ws[s];
        const size_t px_in = s == 0 ? px_out : (size_t)N * p.Hs[s - 1] * p.Ws[s - 1];
        max_out = std::max(max_out, px_out * cout * es);
        max_mid = std::max(max_mid, (c.stride_in_1x1 ? px_out : px_in) * cmid * es);
        cout *= 2;
        cmid *= 2;
    }
    p.bufA = cv.take(max_out);
    p.bufB = cv.take(max_out);
    p.bufSC = cv.take(max_out);
    p.bufT1 = cv.take(max_mid);
    p.bufT2 = cv.take(max_mid);
    const size_t Mf = (size_t)N * p.Hf * p.Wf;
    p.rpn_hid = cv.take(Mf * h->hid * es);
    p.rpn_out = (float *)cv.take(Mf * (size_t)((5 * h->A + 7) / 8 * 8) * sizeof(float));
    p.prop_boxes = (float *)cv.take((size_t)p.K * 4 * sizeof(float));
    p.prop_logits = (float *)cv.take((size_t)p.K * sizeof(float));
    p.rois = (float *)cv.take((size_t)p.K * 5 * sizeof(float));
    p.prop_counts = (int32_t *)cv.take((size_t)N * sizeof(int32_t));
    p.image_hw = (int32_t *)cv.take((size_t)N * 2 * sizeof(int32_t));
    p.scales = (float *)cv.take((size_t)N * 2 * sizeof(float));
    p.nonfinite = (int32_t *)cv.take(sizeof(int32_t));
    p.rpn_ws_bytes = vk_rpn_workspace_bytes(N, p.Hf * p.Wf * h->A, c.pre_nms_topk);
    p.rpn_ws = cv.take(p.rpn_ws_bytes);
    const size_t roi_rows = (size_t)p.chunk * p.P * p.P;
    const size_t rows = whole_map ? std::max(roi_rows, Mf) : roi_rows;
    const int mid5 = c.num_groups * c.width_per_group * 8;
    p.head_rows = rows;
    p.pooled = cv.take(roi_rows * h->res4_c * es);
    p.h_t1 = cv.take(rows * mid5 * es);
    p.h_t2 = cv.take(rows * mid5 * es);
    p.h_a = cv.take(rows * h->res5_c * es);
    p.h_b = cv.take(rows * h->res5_c * es);
    p.h_sc = cv.take(rows * h->res5_c * es);
    if (head_dedupe_planned(h) && !whole_map && p.chunk > 0) {
        const size_t ws = vk_roi_windows_workspace_bytes(N, p.Hf, p.Wf);
        if (ws > 0 && ws <= ((size_t)1 << 30) && roi_rows < ((size_t)1 << 31)) {
            p.dd_ws_bytes = ws;
            p.dd_ws = cv.take(ws);
            p.dd_idx = (int32_t *)cv.take(roi_rows * sizeof(int32_t));
            p.dd_win = (int32_t *)cv.take(roi_rows * 5 * sizeof(int32_t));
            p.dd_u = (int32_t *)cv.take((size_t)ceil_div(p.K, p.chunk) * sizeof(int32_t));
            const size_t nws = h->res5.size() >= 3 ? vk_roi_neighbourhoods_workspace_bytes((long)roi_rows) : 0;
            if (nws > 0) {
                p.nb_ws_bytes = nws;
                p.nb_ws = cv.take(nws);
                p.nb_nid = (int32_t *)cv.take(roi_rows * sizeof(int32_t));
                p.nb_rep = (int32_t *)cv.take(roi_rows * sizeof(int32_t));
                p.nb_idx_rep = (int32_t *)cv.take(roi_rows * sizeof(int32_t));
                p.nb_out_row = (int32_t *)cv.take(roi_rows * sizeof(int32_t));
                p.nb_v = (int32_t *)cv.take((size_t)ceil_div(p.K, p.chunk) * sizeof(int32_t));
            }
        }
    }
    p.pool_part = nullptr;
    // + one tile: two half-chunks on two streams keep separate partials and each rounds its tile count up
    if (fused_mean_ok(h, p.P, roi_rows)) p.pool_part = (float *)cv.take(conv_duo_pool_part_bytes((long)roi_rows + 128, h->res5_c));
    p.feat = (float *)cv.take((size_t)p.K * h->res5_c * sizeof(float));
    const size_t pes = dtype_size(h->pdt);
    p.featT = cv.take((size_t)p.K * h->res5_c * pes);
    p.concat = cv.take((size_t)p.K * (h->res5_c + h->emb_dim) * pes);
    p.attr_hid = cv.take((size_t)p.K * (h->res5_c / 4) * pes);
    p.cls_logits = (float *)cv.take((size_t)p.K * ((c.num_classes + 1 + 7) / 8 * 8) * sizeof(float));
    p.attr_logits = (float *)cv.take((size_t)p.K * ((c.num_attrs + 1 + 7) / 8 * 8) * sizeof(float));
    p.obj_prob = (float *)cv.take((size_t)p.K * sizeof(float));
    p.attr_prob = (float *)cv.take((size_t)p.K * sizeof(float));
    p.chosen = (float *)cv.take((size_t)p.K * 4 * sizeof(float));
    p.obj_cls = (int32_t *)cv.take((size_t)p.K * sizeof(int32_t));
    p.attr_cls = (int32_t *)cv.take((size_t)p.K * sizeof(int32_t));
    p.max_class = (int32_t *)cv.take((size_t)p.K * sizeof(int32_t));
    p.keep_ids = (int64_t *)cv.take((size_t)N * D * sizeof(int64_t));
    p.bands = cv.take((size_t)N * VK_MAX_IGNOREY * 2 * sizeof(double));
    p.band_counts = (int32_t *)cv.take((size_t)N * sizeof(int32_t));
    p.total = cv.off;
    return p;
}

// What a layer's launch may set beyond the layer itself, its input and its output: name what you set, the rest stays off.
struct ConvOpts {
    const void *res = nullptr;      // residual, added before the ReLU
    const void *x2 = nullptr;       // second input of a dual-source 1x1 (the block's input under a fused shortcut), cin2 channels
    int cin2 = 0;
    float *pool_part = nullptr;     // fused spatial mean: the per-tile column sums go here
    bool concurrent = false;        // launched beside another stream's kernels
    int out_dt = -1;                // -1: the layer's own precision
    int ldy = 0;                    // 0: cout rounded up to 8
    bool relu = false;
};

static ConvArgs layer_args(const vk_handle *h, const ConvLayer &L, const void *x, int N, int H, int W, void *y, ConvOpts o) {
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.concurrent = o.concurrent ? 1 : 0;
    a.x = x;
    a.x2 = o.x2;
    a.Cin2 = o.cin2;
    a.pool_part = o.pool_part;
    a.w = L.w;
    a.bias = L.b;
    a.res = o.res;
    a.y = y;
    a.N = N;
    a.H = H;
    a.W = W;
    a.Cin = L.cin;
    conv_out_hw(H, W, L.k, L.stride, L.pad, L.dil, &a.Ho, &a.Wo);
    a.Cout = L.cout;
    a.ldy = o.ldy > 0 ? o.ldy : (L.cout + 7) / 8 * 8;
    a.kh = a.kw = L.k;
    a.stride = L.stride;
    a.pad = L.pad;
    a.dil = L.dil;
    a.groups = L.groups;
    a.relu = o.relu;
    a.stem = 0;
    a.dt = L.dt >= 0 ? (vk_dtype)L.dt : h->dt;
    a.out_dt = o.out_dt >= 0 ? (vk_dtype)o.out_dt : a.dt;
    return a;
}

static int run_conv(vk_handle *h, const ConvLayer &L, const void *x, int N, int H, int W, void *y, hipStream_t s, ConvOpts o,
                    int *Ho = nullptr, int *Wo = nullptr) {
    const ConvArgs a = layer_args(h, L, x, N, H, W, y, o);
    if (Ho) *Ho = a.Ho;
    if (Wo) *Wo = a.Wo;
    return launch_conv(a, s);
}

// BottleneckBlock.forward frcnn.py:963-979.  x [N,H,W,cin] -> y [N,Ho,Wo,cout]
// n0 / nb: run images [n0, n0 + nb) of the full-batch buffers (every buffer is [N, H, W, C]: the half-batch pointers are
// plain offsets).  nb < 0: the whole batch.
static int run_block(vk_handle *h, const Block &b, const void *x, int N, int H, int W, void *t1, void *t2, void *sc,
                     void *y, hipStream_t s, int *Ho, int *Wo, float *pool_part = nullptr, int n0 = 0, int nb = -1) {
    int h1, w1, h2, w2;
    const bool cc = nb >= 0;            // half-batch beside the other half on a second stream
    if (nb >= 0) {
        const size_t es = dtype_size(h->dt);
        int ho, wo;
        conv_out_hw(H, W, b.conv1.k, b.conv1.stride, b.conv1.pad, b.conv1.dil, &h1, &w1);
        conv_out_hw(h1, w1, b.conv2.k, b.conv2.stride, b.conv2.pad, b.conv2.dil, &h2, &w2);
        conv_out_hw(h2, w2, 1, 1, 0, 1, &ho, &wo);
        x = (const char *)x + (size_t)n0 * H * W * b.conv1.cin * es;
        t1 = (char *)t1 + (size_t)n0 * h1 * w1 * b.conv1.cout * es;
        t2 = (char *)t2 + (size_t)n0 * h2 * w2 * b.conv2.cout * es;
        sc = (char *)sc + (size_t)n0 * ho * wo * b.conv3.cout * es;
        y = (char *)y + (size_t)n0 * ho * wo * b.conv3.cout * es;
        N = nb;
    }
    // res2: the whole block as one kernel (bneck_fused.hip) -- x is read once, t1 / t2 never leave the CU
    if (!pool_part && vk_bottleneck64_eligible(b.conv1.cin, b.conv1.cout, b.conv3.cout, b.conv1.stride * b.conv2.stride, b.conv2.dil,
                                               b.conv2.groups, b.has_shortcut, b.fused_shortcut, N, H, W, h->dt)) {
        if (Ho) *Ho = H;
        if (Wo) *Wo = W;
        return launch_bneck_fused(x, N, H, W, b.conv1.cin, b.has_shortcut, b.conv1.w, b.conv1.b, b.conv2.w, b.conv2.b, b.conv3.w, b.conv3.b, y,
                                  cc, s);
    }
    const void *res = x;
    if (b.has_shortcut && !b.fused_shortcut) {
        VK_TRY(run_conv(h, b.shortcut, x, N, H, W, sc, s, {.concurrent = cc}));
        res = sc;
    }
    VK_TRY(run_conv(h, b.conv1, x, N, H, W, t1, s, {.concurrent = cc, .relu = true}, &h1, &w1));
    VK_TRY(run_conv(h, b.conv2, t1, N, h1, w1, t2, s, {.concurrent = cc, .relu = true}, &h2, &w2));
    if (b.fused_shortcut)      // stride-1 block: t2 and x cover the same pixels
        return run_conv(h, b.conv3, t2, N, h2, w2, y, s, {.x2 = x, .cin2 = b.shortcut.cin, .pool_part = pool_part, .concurrent = cc, .relu = true}, Ho, Wo);
    return run_conv(h, b.conv3, t2, N, h2, w2, y, s, {.res = res, .pool_part = pool_part, .concurrent = cc, .relu = true}, Ho, Wo);
}

static void set_stage(vk_handle *h, const char *name, const void *ptr, vk_dtype dt, std::initializer_list<int64_t> shape) {
    vk_handle::Stage st;
    st.ptr = ptr;
    st.dt = dt;
    st.ndim = 0;
    for (auto v : shape) st.shape[st.ndim++] = v;
    h->stages_out[name] = st;
}

}  // namespace vk

extern "C" {

int vk_create(const vk_config *cfg, int device, vk_handle **out) {
    VK_REQUIRE(cfg && out, VK_EINVAL, "create: null argument");
    VK_REQUIRE(cfg->depth == 50 || cfg->depth == 101 || cfg->depth == 152, VK_EINVAL, "create: depth %d unsupported", cfg->depth);
    VK_REQUIRE(cfg->num_groups >= 1 && cfg->width_per_group >= 1 &&
                   (cfg->num_groups == 1 || (cfg->width_per_group & (cfg->width_per_group - 1)) == 0),
               VK_EINVAL, "create: NUM_GROUPS=%d needs WIDTH_PER_GROUP (%d) to be a power of two", cfg->num_groups, cfg->width_per_group);
    // RES5HALVE=false only resets conv1/shortcut strides (frcnn.py:1351-1352): with the stride on conv2 the
    // reference's block 0 adds a 7x7 main path to a 14x14 shortcut and raises
    VK_REQUIRE(cfg->stride_in_1x1 != 0 || cfg->res5_halve != 0, VK_EINVAL,
               "create: STRIDE_IN_1X1=false with RES5HALVE=false leaves a stride-2 conv2 in res5 (frcnn.py:1351-1355): "
               "the reference's residual add fails on the shapes");
    VK_REQUIRE(cfg->precision == VK_F16 || cfg->precision == VK_F32, VK_EINVAL, "create: precision must be VK_F16 or VK_F32");
    VK_REQUIRE(cfg->num_sizes >= 1 && cfg->num_sizes <= VK_MAX_ANCHOR_DIM && cfg->num_ratios >= 1 &&
                   cfg->num_ratios <= VK_MAX_ANCHOR_DIM, VK_EINVAL, "create: bad anchor configuration");
    VK_REQUIRE(cfg->pre_nms_topk >= 1 && cfg->pre_nms_topk <= 8192, VK_EINVAL, "create: PRE_NMS_TOPK_TEST must be in 1..8192");
    VK_REQUIRE(cfg->post_nms_topk >= 1 && cfg->post_nms_topk <= 1024 && cfg->post_nms_topk <= cfg->pre_nms_topk, VK_EINVAL,
               "create: POST_NMS_TOPK_TEST must be in 1..min(1024, PRE_NMS_TOPK_TEST)");
    VK_REQUIRE(cfg->use_attr != 0, VK_EINVAL, "create: ROI_BOX_HEAD.ATTR=false is not supported");
    VK_REQUIRE(cfg->stem_out_channels == 64, VK_EINVAL, "create: STEM_OUT_CHANNELS must be 64");
    VK_CHECK_HIP(hipSetDevice(device));
    vk_handle *h = new vk_handle();
    h->cfg = *cfg;
    h->device = device;
    h->dt = (vk_dtype)cfg->precision;
    if (env_set("VK_PREDICTOR_FP16")) h->pdt = h->dt;           // round 1's 16-bit predictor
    for (const OptionRow &o : kOptions) (void)vk_option_default(o.key, &(h->*o.member));     // the built-in defaults or the VK_* variables
    const int di = cfg->depth == 50 ? 0 : (cfg->depth == 101 ? 1 : 2);
    add_conv_names(h->names, "backbone.stem.conv1", true);
    h->stem = ConvLayer{"backbone.stem.conv1", 3, cfg->stem_out_channels, 7, 2, 3, 1, true, true};
    int cin = cfg->stem_out_channels, cout = cfg->res2_out_channels, cmid = cfg->num_groups * cfg->width_per_group;
    const char *sn[3] = {"res2", "res3", "res4"};
    for (int s = 0; s < 3; ++s) {
        for (int b = 0; b < kBlocks[di][s]; ++b) {
            const int stride = (b == 0 && s > 0) ? 2 : 1;   // frcnn.py:237
            h->stages[s].push_back(make_block(std::string("backbone.") + sn[s] + "." + std::to_string(b), cin, cmid, cout,
                                              stride, 1, cfg->stride_in_1x1 != 0, cfg->num_groups, h->names));
            cin = cout;
        }
        cout *= 2;
        cmid *= 2;
    }
    h->res4_c = cin;
    h->A = cfg->num_sizes * cfg->num_ratios;
    h->names.push_back("proposal_generator.anchor_generator.cell_anchors.0");
    h->hid = cfg->rpn_hidden_channels == -1 ? h->res4_c : cfg->rpn_hidden_channels;
    h->rpn_conv = ConvLayer{"proposal_generator.rpn_head.conv", h->res4_c, h->hid, 3, 1, 1, 1, false, true};
    add_conv_names(h->names, h->rpn_conv.prefix, false);
    add_conv_names(h->names, "proposal_generator.rpn_head.objectness_logits", false);
    add_conv_names(h->names, "proposal_generator.rpn_head.anchor_deltas", false);
    h->rpn_heads = ConvLayer{"proposal_generator.rpn_head.(objectness_logits|anchor_deltas)", h->hid, 5 * h->A, 1, 1, 0, 1, false, false};
    h->res5_c = cfg->res2_out_channels * 8;
    const int mid5 = cfg->num_groups * cfg->width_per_group * 8;
    cin = h->res4_c;
    for (int b = 0; b < 3; ++b) {
        // VG res5 (RES5HALVE=false): stride 1, conv2 dilation/padding 2 (frcnn.py:1345-1355);
        // RES5HALVE=true: the plain stage, first stride 2 (frcnn.py:1373-1383)
        const bool halve = cfg->res5_halve != 0;
        h->res5.push_back(make_block("roi_heads.res5." + std::to_string(b), cin, mid5, h->res5_c, (halve && b == 0) ? 2 : 1,
                                     halve ? 1 : 2, cfg->stride_in_1x1 != 0, cfg->num_groups, h->names));
        cin = h->res5_c;
    }
    const int C = cfg->num_classes, F = h->res5_c;
    h->emb_dim = F / 8;
    const std::string bp = "roi_heads.box_predictor.";
    h->cls_score = ConvLayer{bp + "cls_score", F, C + 1, 1, 1, 0, 1, false, false};
    h->fc_attr = ConvLayer{bp + "fc_attr", F + h->emb_dim, F / 4, 1, 1, 0, 1, false, true};
    h->attr_score = ConvLayer{bp + "attr_score", F / 4, cfg->num_attrs + 1, 1, 1, 0, 1, false, false};
    for (const char *n : {"cls_score", "bbox_pred"}) add_conv_names(h->names, bp + n, false);
    h->names.push_back(bp + "cls_embedding.weight");
    for (const char *n : {"fc_attr", "attr_score"}) add_conv_names(h->names, bp + n, false);
    *out = h;
    return VK_OK;
}

int vk_num_weights(vk_handle *h, int *count) {
    VK_REQUIRE(h && count, VK_EINVAL, "null argument");
    *count = (int)h->names.size();
    return VK_OK;
}

int vk_weight_name(vk_handle *h, int index, const char **name) {
    VK_REQUIRE(h && name && index >= 0 && index < (int)h->names.size(), VK_EINVAL, "weight index out of range");
    *name = h->names[index].c_str();
    return VK_OK;
}

int vk_load_weights(vk_handle *h, const char *name, const void *host_ptr, const int64_t *shape, int ndim, vk_dtype dtype) {
    VK_REQUIRE(h && name && host_ptr && (shape || ndim == 0), VK_EINVAL, "load_weights: null argument");
    VK_REQUIRE(!h->finalized, VK_EINVAL, "load_weights: model already finalized");
    std::string key(name);
    // old -> new naming, as the reference's loader does (frcnn.py:1862-1872)
    size_t pos;
    if ((pos = key.find("gamma")) != std::string::npos) key.replace(pos, 5, "weight");
    if ((pos = key.find("beta")) != std::string::npos) key.replace(pos, 4, "bias");
    if (key.size() > 19 && key.compare(key.size() - 19, 19, "num_batches_tracked") == 0) return VK_OK;   // unused in eval
    bool known = false;
    for (auto &n : h->names) known |= (n == key);
    VK_REQUIRE(known, VK_EWEIGHTS, "unexpected key '%s' in state_dict (strict load)", key.c_str());
    VK_REQUIRE(dtype == VK_F32, VK_EINVAL, "load_weights: '%s' must be float32", key.c_str());
    HostTensor t;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) {
        t.shape.push_back(shape[i]);
        n *= (size_t)shape[i];
    }
    t.data.assign((const float *)host_ptr, (const float *)host_ptr + n);
    t.loaded = true;
    h->host[key] = std::move(t);
    return VK_OK;
}

int vk_finalize(vk_handle *h) {
    VK_REQUIRE(h, VK_EINVAL, "finalize: null handle");
    VK_REQUIRE(!h->finalized, VK_EINVAL, "finalize: already finalized");
    VK_CHECK_HIP(hipSetDevice(h->device));
    for (auto &n : h->names) {
        auto it = h->host.find(n);
        VK_REQUIRE(it != h->host.end() && it->second.loaded, VK_EWEIGHTS, "missing key '%s' in state_dict (strict load)", n.c_str());
    }
    const vk_config &c = h->cfg;
    // stem
    {
        const HostTensor *w = get_t(h, "backbone.stem.conv1.weight", {c.stem_out_channels, 3, 7, 7});
        if (!w) return VK_EWEIGHTS;
        std::vector<float> bn;
        VK_TRY(gather_bn(h, "backbone.stem.conv1", c.stem_out_channels, bn));
        std::vector<char> packed(vk_packed_stem_bytes(c.stem_out_channels, h->dt));
        std::vector<float> pb(vk_packed_cout(c.stem_out_channels));
        VK_TRY(vk_pack_stem_weight(w->data.data(), bn.data(), c.stem_out_channels, h->dt, packed.data(), pb.data()));
        VK_TRY(upload(h, packed.data(), packed.size(), &h->stem.w));
        VK_TRY(upload(h, pb.data(), pb.size() * sizeof(float), (void **)&h->stem.b));
    }
    for (int s = 0; s < 3; ++s)
        for (auto &b : h->stages[s]) VK_TRY(finalize_block(h, b));
    for (auto &b : h->res5) VK_TRY(finalize_block(h, b));
    VK_TRY(finalize_conv(h, h->rpn_conv));
    {   // fuse the two 1x1 RPN heads into one GEMM: rows [0,A) objectness, [A,5A) anchor deltas
        const int A = h->A, hid = h->hid;
        const HostTensor *wo = get_t(h, "proposal_generator.rpn_head.objectness_logits.weight", {A, hid, 1, 1});
        const HostTensor *bo = get_t(h, "proposal_generator.rpn_head.objectness_logits.bias", {A});
        const HostTensor *wd = get_t(h, "proposal_generator.rpn_head.anchor_deltas.weight", {4 * A, hid, 1, 1});
        const HostTensor *bd = get_t(h, "proposal_generator.rpn_head.anchor_deltas.bias", {4 * A});
        if (!wo || !bo || !wd || !bd) return VK_EWEIGHTS;
        std::vector<float> w(wo->data), b(bo->data);
        w.insert(w.end(), wd->data.begin(), wd->data.end());
        b.insert(b.end(), bd->data.begin(), bd->data.end());
        std::vector<char> packed(vk_packed_weight_bytes(5 * A, hid, 1, 1, 1, h->dt));
        std::vector<float> pb(vk_packed_cout(5 * A));
        VK_TRY(vk_pack_conv_weight(w.data(), nullptr, b.data(), 5 * A, hid, 1, 1, 1, h->dt, packed.data(), pb.data()));
        VK_TRY(upload(h, packed.data(), packed.size(), &h->rpn_heads.w));
        VK_TRY(upload(h, pb.data(), pb.size() * sizeof(float), (void **)&h->rpn_heads.b));
        const HostTensor *ca = get_t(h, "proposal_generator.anchor_generator.cell_anchors.0", {A, 4});
        if (!ca) return VK_EWEIGHTS;
        VK_TRY(upload(h, ca->data.data(), ca->data.size() * sizeof(float), (void **)&h->cell_anchors));
    }
    // predictor: Linear weights [out,in] are 1x1 convs [out,in,1,1]
    const std::string bp = "roi_heads.box_predictor.";
    for (ConvLayer *L : {&h->cls_score, &h->fc_attr, &h->attr_score}) {
        auto it = h->host.find(L->prefix + ".weight");
        if (it != h->host.end() && it->second.shape.size() == 2) {
            it->second.shape.push_back(1);
            it->second.shape.push_back(1);
        }
        L->dt = h->pdt;
        VK_TRY(finalize_conv(h, *L));
    }
    {
        const int C = c.num_classes, F = h->res5_c;
        const int nb = c.cls_agnostic_bbox_reg ? 1 : C;
        const HostTensor *w = get_t(h, bp + "bbox_pred.weight", {4 * nb, F});
        const HostTensor *b = get_t(h, bp + "bbox_pred.bias", {4 * nb});
        const HostTensor *e = get_t(h, bp + "cls_embedding.weight", {C + 1, h->emb_dim});
        if (!w || !b || !e) return VK_EWEIGHTS;
        std::vector<char> tmp(w->data.size() * dtype_size(h->pdt));
        to_dt(w->data.data(), w->data.size(), h->pdt, tmp.data());
        VK_TRY(upload(h, tmp.data(), tmp.size(), &h->bbox_w));
        VK_TRY(upload(h, b->data.data(), b->data.size() * sizeof(float), (void **)&h->bbox_b));
        tmp.resize(e->data.size() * dtype_size(h->pdt));
        to_dt(e->data.data(), e->data.size(), h->pdt, tmp.data());
        VK_TRY(upload(h, tmp.data(), tmp.size(), &h->emb));
    }
    h->host.clear();
    h->finalized = true;
    return VK_OK;
}

int vk_option_check(const char *key, int value) {
    VK_REQUIRE(key, VK_EINVAL, "option: null key");
    const OptionRow *o = find_option(key);
    if (!o) return VK_EINVAL;
    VK_REQUIRE(value >= o->lo && value <= o->hi, VK_EINVAL, "%s", o->range_msg);
    return VK_OK;
}

int vk_option_default(const char *key, int *value) {
    VK_REQUIRE(key && value, VK_EINVAL, "option: null argument");
    const OptionRow *o = find_option(key);
    if (!o) return VK_EINVAL;
    *value = o->def;
    const char *env = o->env ? env_text(o->env) : nullptr;
    // (the one option whose variable is named here and not in its row)
    if (o->member == &vk_handle::head_dedupe_taps) env = env_text("VK_HEAD_DEDUPE_TAPS");
    if (!env) return VK_OK;
    if (o->rule == ENV_ATOI_POSITIVE) {
        if (atoi(env) > 0) *value = atoi(env);
    } else if (env[0] >= '0' + o->lo && env[0] <= '0' + o->hi && (o->rule == ENV_FIRST_DIGIT || !env[1])) {
        *value = env[0] - '0';
    }
    return VK_OK;
}

int vk_get_option(vk_handle *h, const char *key, int *value) {
    VK_REQUIRE(h && key && value, VK_EINVAL, "get_option: null argument");
    for (const OptionRow &o : kOptions)
        if (!strcmp(key, o.key)) {
            *value = h->*o.member;
            return VK_OK;
        }
    // read-only
    if (!strcmp(key, "dedupe_chunks")) *value = (int)std::min<int64_t>(h->dedupe_chunks, INT32_MAX);      // head chunks that took the dedupe path
    else if (!strcmp(key, "indexed_chunks")) *value = (int)std::min<int64_t>(h->indexed_chunks, INT32_MAX);   // ... and ran conv2 without the row gather
    else if (!strcmp(key, "tap_dedupe_chunks")) *value = (int)std::min<int64_t>(h->tap_dedupe_chunks, INT32_MAX);   // ... and went on over the distinct neighbourhoods
    else if (!strcmp(key, "out_indexed_chunks")) *value = (int)std::min<int64_t>(h->out_indexed_chunks, INT32_MAX);   // ... with conv2 of block 0 storing the distinct rows itself
    else if (!strcmp(key, "working_sets")) *value = (h->sets[0].arena ? 1 : 0) + (h->sets[1].arena ? 1 : 0);   // arenas held
    else if (!strcmp(key, "lane_forwards")) *value = (int)std::min<int64_t>(h->lane_forwards, INT32_MAX);    // forwards enqueued on a lane's stream
    else VK_REQUIRE(false, VK_EINVAL, "unknown option '%s'", key);
    return VK_OK;
}

int vk_set_option(vk_handle *h, const char *key, int value) {
    VK_REQUIRE(h && key, VK_EINVAL, "set_option: null argument");
    VK_TRY(vk_option_check(key, value));
    h->*find_option(key)->member = value;
    return VK_OK;
}

int vk_pooler_check(int type, int sampling_ratio) {
    VK_REQUIRE(type == VK_POOLER_ROIPOOL || type == VK_POOLER_ROIALIGN || type == VK_POOLER_ROIALIGNV2, VK_EINVAL,
               "pooler type %d must be VK_POOLER_ROIPOOL, VK_POOLER_ROIALIGN or VK_POOLER_ROIALIGNV2", type);
    VK_REQUIRE(sampling_ratio >= 0 && sampling_ratio <= 8, VK_EINVAL, "POOLER_SAMPLING_RATIO %d must be in 0..8 (0 = adaptive)", sampling_ratio);
    return VK_OK;
}

int vk_set_pooler(vk_handle *h, int type, int sampling_ratio) {
    VK_REQUIRE(h, VK_EINVAL, "set_pooler: null handle");
    VK_TRY(vk_pooler_check(type, sampling_ratio));
    VK_REQUIRE(h->next_ticket == 0, VK_EINVAL, "set_pooler: the pooler is fixed once the handle has run a forward");
    h->pooler_type = type;
    h->pooler_sampling_ratio = sampling_ratio;
    return VK_OK;
}

int vk_get_pooler(vk_handle *h, int *type, int *sampling_ratio) {
    VK_REQUIRE(h && type && sampling_ratio, VK_EINVAL, "get_pooler: null argument");
    *type = h->pooler_type;
    *sampling_ratio = h->pooler_sampling_ratio;
    return VK_OK;
}

int vk_destroy(vk_handle *h) {
    if (!h) return VK_OK;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    for (void *p : h->owned) (void)hipFree(p);
    for (auto &ws : h->sets) {
        if (ws.arena) (void)hipFree(ws.arena);
        if (ws.pc_arena) (void)hipFree(ws.pc_arena);
        if (ws.det_arena) (void)hipFree(ws.det_arena);
    }
    for (auto &e : h->ev)
        if (e) (void)hipEventDestroy(e);
    for (auto &e : h->ev_done)
        if (e) (void)hipEventDestroy(e);
    for (auto &e : h->ev_in)
        if (e) (void)hipEventDestroy(e);
    if (h->flag_host) (void)hipHostFree(h->flag_host);
    if (h->meta_host) (void)hipHostFree(h->meta_host);
    for (auto &ln : h->lanes) {
        if (ln.ev_fork) (void)hipEventDestroy(ln.ev_fork);
        if (ln.ev_join) (void)hipEventDestroy(ln.ev_join);
        for (auto &e : ln.more_joins)
            if (e) (void)hipEventDestroy(e);
        if (ln.main) (void)hipStreamDestroy(ln.main);
    }
    if (h->side) (void)hipStreamDestroy(h->side);
    for (auto &st : h->more_sides)
        if (st) (void)hipStreamDestroy(st);
    delete h->ktimer;
    delete h;
    return VK_OK;
}

int vk_enable_stage_timing(vk_handle *h, int enable) {
    VK_REQUIRE(h, VK_EINVAL, "null handle");
    h->timing = enable != 0;
    if (h->timing && !h->ev[0])
        for (auto &e : h->ev) VK_CHECK_HIP(hipEventCreate(&e));
    return VK_OK;
}

int vk_get_stage_timing(vk_handle *h, float *ms6) {
    VK_REQUIRE(h && ms6, VK_EINVAL, "null argument");
    VK_REQUIRE(h->timing && h->ev_valid, VK_EINVAL, "stage timing was not recorded");
    VK_CHECK_HIP(hipEventSynchronize(h->ev[5]));
    for (int i = 0; i < 5; ++i) VK_CHECK_HIP(hipEventElapsedTime(&ms6[i], h->ev[i], h->ev[i + 1]));
    VK_CHECK_HIP(hipEventElapsedTime(&ms6[5], h->ev[0], h->ev[5]));
    return VK_OK;
}

int vk_get_stage(vk_handle *h, const char *name, const void **dev_ptr, vk_dtype *dtype, int64_t *shape, int *ndim) {
    VK_REQUIRE(h && name && dev_ptr && dtype && shape && ndim, VK_EINVAL, "null argument");
    auto it = h->stages_out.find(name);
    VK_REQUIRE(it != h->stages_out.end(), VK_EINVAL, "unknown stage '%s' (or no forward has run)", name);
    // the stages are the most recently begun forward's, in its working set; where that forward is still open on a lane's
    // stream, a copy on the caller's stream would not be ordered behind it
    if (h->next_ticket > h->oldest_open) {
        const int slot = (int)((h->next_ticket - 1) % vk_handle::VK_MAX_INFLIGHT);
        if (h->slot_stream[slot] != h->slot_caller[slot]) VK_CHECK_HIP(hipEventSynchronize(h->ev_done[slot]));
    }
    // "pooled" of a forward that pooled each distinct window once: the dense tensor is built now, on the stream that forward's
    // caller passed (ordered behind the forward there: it ran on that stream, has been waited for above, or has ended)
    if (h->pooled_expand.pending && !strcmp(name, "pooled") && h->next_ticket > 0) {
        const auto &e = h->pooled_expand;
        const int slot = (int)((h->next_ticket - 1) % vk_handle::VK_MAX_INFLIGHT);
        VK_TRY(vk_gather_rows(e.src, e.idx, e.rows, e.row_bytes, e.dst, h->slot_caller[slot]));
        h->pooled_expand.pending = false;
    }
    *dev_ptr = it->second.ptr;
    *dtype = it->second.dt;
    *ndim = it->second.ndim;
    for (int i = 0; i < it->second.ndim; ++i) shape[i] = it->second.shape[i];
    return VK_OK;
}

int vk_forward(vk_handle *h, const float *images_dev, int N, int H, int W, const int32_t *image_hw,
               const float *scales_yx, const vk_roi_params *rp, const vk_outputs *out, void *stream) {
    int64_t ticket = -1;
    VK_TRY(vk_forward_begin(h, images_dev, N, H, W, image_hw, scales_yx, rp, out, stream, &ticket));
    return vk_forward_end(h, ticket);
}

}  // extern "C"

namespace vk {

// ---- the pieces of a forward shared by vk_forward_begin (detection) and vk_forward_boxes_begin (given boxes) ----

// The pinned flag words and the per-ticket events, on the first forward.
static int ensure_ticket_state(vk_handle *h) {
    if (h->flag_host) return VK_OK;
    for (auto &e : h->ev_done) VK_CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto &e : h->ev_in) VK_CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    VK_CHECK_HIP(hipHostMalloc((void **)&h->flag_host, sizeof(int32_t) * vk_handle::VK_MAX_INFLIGHT, hipHostMallocDefault));
    return VK_OK;
}

// A device block of at least `need` bytes: the arenas of a working set grow through this.  Growing frees the old block after
// hipDeviceSynchronize, which also waits for a forward in flight on the other set (it keeps its own blocks).  soft: a failed
// allocation is reported as 1 with the HIP error cleared, not as an error.
static int grow_device_block(char **p, size_t *bytes, size_t need, bool soft) {
    if (need <= *bytes) return VK_OK;
    if (*p) {
        VK_CHECK_HIP(hipDeviceSynchronize());
        VK_CHECK_HIP(hipFree(*p));
        *p = nullptr;
        *bytes = 0;
    }
    if (soft) {
        if (hipMalloc((void **)p, need) != hipSuccess) {
            (void)hipGetLastError();
            *p = nullptr;
            return 1;
        }
    } else {
        VK_CHECK_HIP(hipMalloc((void **)p, need));
    }
    *bytes = need;
    return VK_OK;
}

static int ensure_arena(vk_handle *h, int set, size_t bytes, bool soft) {
    return grow_device_block(&h->sets[set].arena, &h->sets[set].arena_bytes, bytes, soft);
}

// Where the forward that is about to be enqueued (ticket h->next_ticket) runs: its working set (h->cur_set, with an arena
// of arena_need bytes) and its stream (*s_out).
// One lane (option forward_lanes = 1, timers on, no forward has overlapped another yet, or the second arena did not fit):
// set 0 on the caller's stream, as a handle with one arena does.  The per-launch and per-stage timers need this: their
// event pairs bracket launches whose durations must not overlap.
// Two lanes: ticket t takes set t & 1 and the lane's own stream, which waits for the caller's stream as it stands now
// (inputs ready); vk_forward_end makes the caller's stream wait for the ticket's completion event in turn.
// Either way the stream waits for every open ticket that was enqueued on another stream and shares the set (one lane:
// every such ticket), so a change of mode between two forwards stays ordered.  Tickets that have ended are complete.
static int fwd_route(vk_handle *h, size_t arena_need, hipStream_t caller, hipStream_t *s_out) {
    VK_TRY(ensure_ticket_state(h));
    const int64_t t = h->next_ticket;
    const int slot = (int)(t % vk_handle::VK_MAX_INFLIGHT);
    bool laned = h->forward_lanes == 2 && !h->two_sets_failed && !h->ktimer && !h->timing;
    if (laned && !h->two_sets && t > h->oldest_open) h->two_sets = true;
    laned = laned && h->two_sets;
    int set = laned ? (int)(t & 1) : 0;
    if (set == 1 && ensure_arena(h, 1, arena_need, true) != VK_OK) {      // no room for a second set: not an error
        h->two_sets_failed = true;
        laned = false;
        set = 0;
    }
    VK_TRY(ensure_arena(h, set, arena_need, false));
    hipStream_t s = caller;
    if (laned) {
        vk_handle::Lane &ln = h->lanes[set];
        // (both lanes at the default priority: the second one at the lowest measured the same)
        if (!ln.main) VK_CHECK_HIP(hipStreamCreateWithFlags(&ln.main, hipStreamNonBlocking));
        s = ln.main;
        h->lane_forwards++;
        VK_CHECK_HIP(hipEventRecord(h->ev_in[slot], caller));
        VK_CHECK_HIP(hipStreamWaitEvent(s, h->ev_in[slot], 0));
    }
    for (int64_t u = h->oldest_open; u < t; ++u) {
        const int us = (int)(u % vk_handle::VK_MAX_INFLIGHT);
        if (h->slot_stream[us] == s || (laned && h->slot_set[us] != set)) continue;
        VK_CHECK_HIP(hipStreamWaitEvent(s, h->ev_done[us], 0));
    }
    h->cur_set = set;
    h->cur_caller = caller;
    *s_out = s;
    return VK_OK;
}

// Arena for R RoI rows per image, the stage map cleared, the caller's host arrays copied into the ticket's pinned slot
// (consumed before _begin returns, and the host-to-device copies are truly asynchronous), the non-finite flag zeroed.
// counts (given boxes only): host [N] -> p.prop_counts.  ig (detection only; host arrays, checked by the caller, or null):
// its counts -> p.band_counts, its [N][max_per_image][2] bands -> p.bands.
// `caller` is the stream the caller passed; *s_out is the stream the forward is enqueued on (fwd_route).
static int fwd_open(vk_handle *h, int N, int H, int W, int R, int D, const int32_t *image_hw, const float *scales_yx,
                    const int32_t *counts, const vk_ignorey *ig, hipStream_t caller, Plan *out, hipStream_t *s_out,
                    bool whole_map = false) {
    Plan need = make_plan(h, nullptr, N, H, W, D, R, whole_map);
    VK_TRY(fwd_route(h, need.total, caller, s_out));
    hipStream_t s = *s_out;
    Plan &p = *out;
    p = make_plan(h, h->sets[h->cur_set].arena, N, H, W, D, R, whole_map);
    h->stages_out.clear();
    h->pooled_expand.pending = false;
    if (h->timing) VK_CHECK_HIP(hipEventRecord(h->ev[0], s));

    // slot layout: image_hw [N,2] i32 | scales_yx [N,2] f32 | counts [N] i32 | band counts [N] i32 | (8-aligned) bands
    const size_t hw_bytes = sizeof(int32_t) * 2 * (size_t)N, sc_bytes = sizeof(float) * 2 * (size_t)N;
    const size_t cnt_bytes = sizeof(int32_t) * (size_t)N;
    const size_t band_off = align_up(hw_bytes + sc_bytes + 2 * cnt_bytes, 8);
    const size_t band_bytes = ig ? (size_t)N * ig->max_per_image * 2 * (ig->f64 ? sizeof(double) : sizeof(float)) : 0;
    const size_t meta_need = ig ? band_off + band_bytes : hw_bytes + sc_bytes + cnt_bytes;
    if (meta_need > h->meta_cap) {
        VK_CHECK_HIP(hipDeviceSynchronize());
        if (h->meta_host) VK_CHECK_HIP(hipHostFree(h->meta_host));
        h->meta_host = nullptr;
        h->meta_cap = align_up(meta_need, 4096);
        VK_CHECK_HIP(hipHostMalloc((void **)&h->meta_host, h->meta_cap * vk_handle::VK_MAX_INFLIGHT, hipHostMallocDefault));
    }
    char *meta = h->meta_host + (size_t)(h->next_ticket % vk_handle::VK_MAX_INFLIGHT) * h->meta_cap;
    memcpy(meta, image_hw, hw_bytes);
    VK_CHECK_HIP(hipMemcpyAsync(p.image_hw, meta, hw_bytes, hipMemcpyHostToDevice, s));
    if (scales_yx) {
        memcpy(meta + hw_bytes, scales_yx, sc_bytes);
        VK_CHECK_HIP(hipMemcpyAsync(p.scales, meta + hw_bytes, sc_bytes, hipMemcpyHostToDevice, s));
    }
    if (counts) {
        memcpy(meta + hw_bytes + sc_bytes, counts, sizeof(int32_t) * (size_t)N);
        VK_CHECK_HIP(hipMemcpyAsync(p.prop_counts, meta + hw_bytes + sc_bytes, sizeof(int32_t) * (size_t)N, hipMemcpyHostToDevice, s));
    }
    if (ig) {
        memcpy(meta + hw_bytes + sc_bytes + cnt_bytes, ig->counts, cnt_bytes);
        VK_CHECK_HIP(hipMemcpyAsync(p.band_counts, meta + hw_bytes + sc_bytes + cnt_bytes, cnt_bytes, hipMemcpyHostToDevice, s));
        memcpy(meta + band_off, ig->bands, band_bytes);
        VK_CHECK_HIP(hipMemcpyAsync(p.bands, meta + band_off, band_bytes, hipMemcpyHostToDevice, s));
    }
    VK_CHECK_HIP(hipMemsetAsync(p.nonfinite, 0, sizeof(int32_t), s));
    return VK_OK;
}

// The handle's side streams (shared by the lanes) and the lane's fork / join events for a split into ns streams.
static int ensure_sides(vk_handle *h, vk_handle::Lane &ln, int ns) {
    if (!h->side) VK_CHECK_HIP(hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking));
    if (!ln.ev_fork) {
        VK_CHECK_HIP(hipEventCreateWithFlags(&ln.ev_fork, hipEventDisableTiming));
        VK_CHECK_HIP(hipEventCreateWithFlags(&ln.ev_join, hipEventDisableTiming));
    }
    for (int i = 0; i < ns - 2; ++i) {
        if (!h->more_sides[i]) VK_CHECK_HIP(hipStreamCreateWithFlags(&h->more_sides[i], hipStreamNonBlocking));
        if (!ln.more_joins[i]) VK_CHECK_HIP(hipEventCreateWithFlags(&ln.more_joins[i], hipEventDisableTiming));
    }
    return VK_OK;
}

// backbone (ResNet.forward frcnn.py:1076-1090): images -> res4 (stage "res4"), then the stage event ev[1]
static int fwd_backbone(vk_handle *h, const Plan &p, const float *images_dev, hipStream_t s, const void **res4_out) {
    const vk_config &c = h->cfg;
    const int N = p.N;
    vk_handle::Lane &ln = h->lanes[h->cur_set];
    VK_TRY(stem_impl(images_dev, N, p.H, p.W, h->stem.w, h->stem.b, c.stem_out_channels, c.caffe_maxpool, p.bufA, h->dt,
                     p.img_pad, p.stem_out, s, p.nonfinite));
    void *cur = p.bufA, *nxt = p.bufB;
    int ch = p.Hs[0], cw = p.Ws[0];
    // res4 at batch 32 is 2.05 rounds of tiles on 256 CUs: every N = 256 layer pays 3 rounds.  Its two half-batches run on
    // two streams, so the tail of one half's layer k overlaps the other half's layer k (images are independent; the
    // halves touch disjoint parts of every buffer).  Option backbone_streams = 1 / VK_BACKBONE_STREAMS=1 disables it.
    for (int st = 0; st < 3; ++st) {
        const bool split = h->backbone_streams >= 2 && st >= 1 && N >= h->backbone_streams && N >= h->backbone_split_min_batch && h->dt == VK_F16;
        const int ns = split ? h->backbone_streams : 1;      // image groups, one stream each
        hipStream_t gs_[4] = {s, nullptr, nullptr, nullptr};
        hipEvent_t gj_[4] = {nullptr, nullptr, nullptr, nullptr};
        if (split) {
            VK_TRY(ensure_sides(h, ln, ns));
            gs_[1] = h->side;
            gj_[1] = ln.ev_join;
            for (int i = 2; i < ns; ++i) {
                gs_[i] = h->more_sides[i - 2];
                gj_[i] = ln.more_joins[i - 2];
            }
            VK_CHECK_HIP(hipEventRecord(ln.ev_fork, s));
            for (int i = 1; i < ns; ++i) VK_CHECK_HIP(hipStreamWaitEvent(gs_[i], ln.ev_fork, 0));
        }
        for (auto &b : h->stages[st]) {
            int ho, wo;
            if (split) {
                for (int i = 0; i < ns; ++i) {
                    const int n0 = (int)((long)N * i / ns), n1 = (int)((long)N * (i + 1) / ns);
                    VK_TRY(run_block(h, b, cur, N, ch, cw, p.bufT1, p.bufT2, p.bufSC, nxt, gs_[i], &ho, &wo, nullptr, n0, n1 - n0));
                }
            } else {
                VK_TRY(run_block(h, b, cur, N, ch, cw, p.bufT1, p.bufT2, p.bufSC, nxt, s, &ho, &wo));
            }
            std::swap(cur, nxt);
            ch = ho;
            cw = wo;
        }
        if (split) {
            for (int i = 1; i < ns; ++i) {
                VK_CHECK_HIP(hipEventRecord(gj_[i], gs_[i]));
                VK_CHECK_HIP(hipStreamWaitEvent(s, gj_[i], 0));
            }
        }
    }
    VK_REQUIRE(ch == p.Hf && cw == p.Wf, VK_EINVAL, "internal: res4 geometry mismatch (%dx%d vs %dx%d)", ch, cw, p.Hf, p.Wf);
    *res4_out = cur;
    set_stage(h, "res4", cur, h->dt, {N, p.Hf, p.Wf, h->res4_c});
    if (h->timing) VK_CHECK_HIP(hipEventRecord(h->ev[1], s));
    return VK_OK;
}

// RoI pool + Res5 head + spatial mean over the p.K rows of p.rois (Res5ROIHeads.forward frcnn.py:1391-1403, chunked over
// RoIs), then the class / attribute branches of the box predictor (FastRCNNOutputLayers.forward frcnn.py:1726-1740; the
// box regression is the caller's: fwd_predictor).  Stages "pooled" (one chunk only), "feature_pooled", "obj_logits", "attr_logits".
static int fwd_predictor(vk_handle *h, const Plan &p, hipStream_t s);

// Res5 block 0 of the chunk of kc RoIs at row k0, each distinct RoIPool window pooled and run through conv1 once (roi_windows.hip,
// DESIGN.md 6c): window table -> pool of the U distinct windows -> conv1 over U rows (M read on the device) -> gather into the dense
// [kc, P, P, mid] input of conv2 -> conv2 -> the fused conv3 + shortcut GEMM, whose second input is pooled_u[idx].  Every row of
// the output h_a goes through the same kernels with the same K order as on the plain path, so it has the same bits.
// Where the whole conv2 launch takes the panel kernel's indexed form (kc a multiple of 16, no panel switch off) there
// is no gather: conv2 reads t1_u[idx[m]] itself.  conv2 writes h_t2, so t1_u then lives in h_t1, which the gather no longer fills;
// h_t1 and h_t2 have the same size (make_plan: a chunk's dense rows), so a chunk without one repeated window (U == rows) still fits.
//
// head_dedupe_taps: block 0's output row, its shortcut operand and conv1 of block 1 depend on the bin's nine-window
// neighbourhood alone, so from conv2 on the 1x1 GEMMs run over the chunk's V distinct neighbourhoods (vk_roi_neighbourhoods; V stays
// on the device).  The table is a function of the boxes alone, so it is built AHEAD of conv2, and conv2 stores each neighbourhood's
// representative row, and no other, straight into t2_v through out_row (the panel kernel's indexed output rows, DESIGN.md 6i;
// t2_v in h_t2: conv2 reads t1_u from h_t1).  The fused conv3 + shortcut GEMM writes Y0_v [V, 2048] into h_a, conv1 of block 1 writes
// t1_v [V, 512] into h_t1 (t1_u is dead behind conv2), conv2 of block 1 reads t1_v through nid (the panel kernel's indexed form) and
// writes its dense t2 into h_t2 (t2_v is dead behind the fused GEMM), and conv3 of block 1 takes its residual from Y0_v through nid
// (conv_ws's indexed-residual build) and writes the dense Y1 into h_b.  Each row goes through the same kernels with the same K
// order as on the path above: same bits.  *block1_done tells fwd_head that block 1 has run.  Taken where conv2 of block 0 took the
// indexed form, Res5 has a block behind block 1 (whose conv3 then stores: the last block's feeds the fused mean) and block 1's three
// layers run as conv_gemm4 (decided at the chunk's dense row count) / the indexed panel form / conv_ws's indexed-residual build.
// Where conv2 cannot store through an index (conv3x3_panel_out_indexed: VK_PANEL_OUT_INDEXED=0) it writes the dense t2 into h_t2
// and vk_gather_rows_dev copies the representative rows into t2_v (h_t1), t1_v then lives in h_t2 and block 1's t2 in h_t1: the
// path of DESIGN.md 6h, same bits.
static bool head_taps_ok(const vk_handle *h, const Plan &p, int kc) {
    if (!h->head_dedupe_taps || !p.nb_nid || h->res5.size() < 3) return false;
    const Block &b1 = h->res5[1];
    const int P = p.P;
    if (b1.has_shortcut || b1.conv1.stride != 1 || b1.conv2.stride != 1 || b1.conv1.cin != h->res5[0].conv3.cout) return false;
    const ConvArgs a1 = layer_args(h, b1.conv1, p.h_a, 1, 1, kc * P * P, p.h_t2, {.relu = true});
    const ConvArgs a2 = layer_args(h, b1.conv2, p.h_t2, kc, P, P, p.h_t1, {.relu = true});
    const ConvArgs a3 = layer_args(h, b1.conv3, p.h_t1, 1, 1, kc * P * P, p.h_b, {.res = p.h_a, .relu = true});
    return conv_route(a1) == VK_ROUTE_GEMM4 && conv_route(a2) == VK_ROUTE_PANEL && conv3x3_panel_phase_indexed(a2) == 1 &&
           conv_route(a3) == VK_ROUTE_WS && conv_ws_res_indexed(a3);
}

static int head_block0_dedupe(vk_handle *h, const Plan &p, const void *res4, int k0, int kc, hipStream_t s, bool *block1_done) {
    const Block &b = h->res5[0];
    const int P = p.P;
    const long rows = (long)kc * P * P;
    const size_t es = dtype_size(h->dt);
    int32_t *u = p.dd_u + k0 / p.chunk;
    ConvArgs a2 = layer_args(h, b.conv2, p.h_t1, kc, P, P, p.h_t2, {.relu = true});
    const bool indexed = conv_route(a2) == VK_ROUTE_PANEL && conv3x3_panel_phase_indexed(a2) == 1;
    void *pooled_u = p.h_sc, *t1_u = indexed ? p.h_t1 : p.h_t2;
    VK_TRY(vk_roi_windows(p.rois + 5 * (size_t)k0, kc, p.N, p.Hf, p.Wf, P, 1.0f / 16.0f, p.dd_idx, p.dd_win, u, p.dd_ws, p.dd_ws_bytes, s));
    VK_TRY(vk_roi_pool_windows(res4, p.N, p.Hf, p.Wf, h->res4_c, p.dd_win, u, (int)rows, pooled_u, h->dt, s));
    ConvArgs a1 = layer_args(h, b.conv1, pooled_u, 1, 1, (int)rows, t1_u, {.relu = true});
    a1.m_dev = u;
    VK_TRY(launch_conv_gemm4(a1, s));
    if (indexed) {
        a2.x_idx = p.dd_idx;
        a2.x_rows = rows;              // (U <= rows is on the device; every index is below U)
        h->indexed_chunks++;
    } else
        VK_TRY(vk_gather_rows(t1_u, p.dd_idx, rows, (int)(b.conv1.cout * es), p.h_t1, s));
    *block1_done = indexed && head_taps_ok(h, p, kc);
    const bool out_indexed = *block1_done && p.nb_out_row && conv3x3_panel_out_indexed(a2) == 1;
    int32_t *v = p.nb_v ? p.nb_v + k0 / p.chunk : nullptr;
    if (*block1_done) VK_TRY(vk_roi_neighbourhoods(p.dd_idx, kc, P, b.conv2.dil, p.nb_nid, p.nb_rep, p.nb_idx_rep, v, p.nb_ws, p.nb_ws_bytes, s));
    if (out_indexed) {
        VK_TRY(vk_roi_out_rows(p.nb_nid, p.nb_rep, rows, p.nb_out_row, s));
        a2.y_idx = p.nb_out_row;
        a2.y_rows = rows;              // (V <= rows is on the device; every entry is -1 or an id below V)
        h->out_indexed_chunks++;
    }
    VK_TRY(launch_conv(a2, s));
    if (*block1_done) {
        const Block &b1 = h->res5[1];
        // out_indexed: conv2 has written t2_v into h_t2; otherwise the dense t2 is there and its representative rows are gathered into h_t1
        void *t2_v = out_indexed ? p.h_t2 : p.h_t1, *y0_v = p.h_a, *t1_v = out_indexed ? p.h_t1 : p.h_t2, *t2_1 = out_indexed ? p.h_t2 : p.h_t1;
        if (!out_indexed) VK_TRY(vk_gather_rows_dev(p.h_t2, p.nb_rep, rows, v, (int)(b.conv2.cout * es), t2_v, s));
        ConvArgs a3 = layer_args(h, b.conv3, t2_v, 1, 1, (int)rows, y0_v, {.x2 = pooled_u, .cin2 = b.shortcut.cin, .relu = true});
        a3.x2_idx = p.nb_idx_rep;
        a3.m_dev = v;
        VK_TRY(launch_conv_gemm4(a3, s));
        ConvArgs c1 = layer_args(h, b1.conv1, y0_v, 1, 1, (int)rows, t1_v, {.relu = true});
        c1.m_dev = v;
        VK_TRY(launch_conv_gemm4(c1, s));
        ConvArgs c2 = layer_args(h, b1.conv2, t1_v, kc, P, P, t2_1, {.relu = true});
        c2.x_idx = p.nb_nid;
        c2.x_rows = rows;                  // (V <= rows is on the device; every id is below V)
        VK_TRY(launch_conv(c2, s));
        ConvArgs c3 = layer_args(h, b1.conv3, t2_1, 1, 1, (int)rows, p.h_b, {.res = y0_v, .relu = true});
        c3.res_idx = p.nb_nid;
        VK_TRY(launch_conv(c3, s));
        h->tap_dedupe_chunks++;
    } else {
        ConvArgs a3 = layer_args(h, b.conv3, p.h_t2, 1, 1, (int)rows, p.h_a, {.x2 = pooled_u, .cin2 = b.shortcut.cin, .relu = true});
        a3.x2_idx = p.dd_idx;
        VK_TRY(launch_conv_gemm4(a3, s));
    }
    h->dedupe_chunks++;
    if (p.chunk >= p.K) {
        h->pooled_expand.pending = true;
        h->pooled_expand.src = pooled_u;
        h->pooled_expand.idx = p.dd_idx;
        h->pooled_expand.rows = rows;
        h->pooled_expand.row_bytes = (int)(h->res4_c * es);
        h->pooled_expand.dst = p.pooled;
    }
    return VK_OK;
}

// The handle's box pooler on nb RoI rows: RoIPool (frcnn.py:1179), or RoIAlign through the pyramid kernel on one level (res4).
// A C4-shaped LDS-staged kernel was measured against it and lost.
static int head_pool(vk_handle *h, const Plan &p, const void *res4, const float *rois, int nb, void *pooled, hipStream_t s) {
    const float scale = 1.0f / 16.0f;
    if (h->pooler_type == VK_POOLER_ROIPOOL) return vk_roi_pool(res4, p.N, p.Hf, p.Wf, h->res4_c, rois, nb, scale, p.P, pooled, h->dt, s);
    const int32_t Hf = p.Hf, Wf = p.Wf;
    return vk_roi_align(&res4, &Hf, &Wf, &scale, 1, p.N, h->res4_c, rois, nullptr, nb, p.P, h->pooler_sampling_ratio,
                        h->pooler_type == VK_POOLER_ROIALIGNV2, pooled, h->dt, s);
}

static int fwd_head(vk_handle *h, const Plan &p, const void *res4, hipStream_t s) {
    const int P = p.P;
    vk_handle::Lane &ln = h->lanes[h->cur_set];
    const size_t es5 = dtype_size(h->dt);
    int dd_chunks = 0, tap_chunks = 0;
    for (int k0 = 0; k0 < p.K; k0 += p.chunk) {
        const int kc = std::min(p.chunk, p.K - k0);
        // option head_streams = 2: the chunk's two halves run on two streams (RoIs are independent; the halves use disjoint
        // rows of every head buffer).  Measured +0.9 % end to end at 9600 RoIs (tails of 58-round launches overlap); starting
        // the second half one or two layers late, so that a 3x3 MFMA loop runs beside a memory-bound 1x1 epilogue, is 1.5 %
        // SLOWER than one stream.  Off by default: it buys little and makes per-kernel durations overlap.
        const bool split = h->head_streams == 2 && kc >= 2 && kc >= h->head_split_min_rois && h->dt == VK_F16;
        const int ka = split ? kc / 2 : kc;
        if (split) {
            VK_TRY(ensure_sides(h, ln, 2));
            VK_CHECK_HIP(hipEventRecord(ln.ev_fork, s));
            VK_CHECK_HIP(hipStreamWaitEvent(h->side, ln.ev_fork, 0));
        }
        const void *x = p.pooled;
        int hh = P, ww = P;
        // Res5 block 0 over the chunk's distinct RoIPool windows (head_block0_dedupe) where its two GEMMs take conv_gemm4 at this
        // chunk size; the plain path otherwise
        bool dd = p.dd_idx && !split && head_dedupe_planned(h);
        if (dd) {
            const Block &b0 = h->res5[0];
            const ConvArgs a1 = layer_args(h, b0.conv1, p.h_sc, 1, 1, kc * P * P, p.h_t2, {.relu = true});
            const ConvArgs a3 = layer_args(h, b0.conv3, p.h_t2, 1, 1, kc * P * P, p.h_a, {.x2 = p.h_sc, .cin2 = b0.shortcut.cin, .relu = true});
            dd = conv_route(a1) == VK_ROUTE_GEMM4 && conv_route(a3) == VK_ROUTE_GEMM4;
        }
        for (int half = 0; half < (split ? 2 : 1); ++half) {
            const int n0 = half ? ka : 0, nb = half ? kc - ka : ka;
            hipStream_t hs = half ? h->side : s;
            bool block1_done = false;
            if (dd) {
                VK_TRY(head_block0_dedupe(h, p, res4, k0, kc, hs, &block1_done));
                dd_chunks++;
                tap_chunks += block1_done ? 1 : 0;
            } else
                VK_TRY(head_pool(h, p, res4, p.rois + 5 * (size_t)(k0 + n0), nb, (char *)p.pooled + (size_t)n0 * P * P * h->res4_c * es5, hs));
            // the fused mean's per-tile partials: the second half gets its own region (tiles are counted per launch)
            float *pp = p.pool_part ? (float *)((char *)p.pool_part + (half ? conv_duo_pool_part_bytes((long)ka * P * P, h->res5_c) : 0)) : nullptr;
            void *a = p.h_a, *b2 = p.h_b;
            x = p.pooled;
            hh = P;
            ww = P;
            if (dd) {              // block 0 has written h_a (stride 1: the map stays P x P)
                x = a;
                std::swap(a, b2);
            }
            if (block1_done) {     // ... and block 1 h_b
                x = a;
                std::swap(a, b2);
            }
            for (size_t bi = dd ? (block1_done ? 2 : 1) : 0; bi < h->res5.size(); ++bi) {
                int ho, wo;
                const bool last = bi + 1 == h->res5.size();
                VK_TRY(run_block(h, h->res5[bi], x, kc, hh, ww, p.h_t1, p.h_t2, p.h_sc, a, hs, &ho, &wo, last ? pp : nullptr,
                                 split ? n0 : 0, split ? nb : -1));
                hh = ho;
                ww = wo;
                x = a;
                std::swap(a, b2);
            }
            if (p.pool_part)
                VK_TRY(launch_pool_finish(pp, nb, hh * ww, h->res5.back().conv3.cin, h->res5_c, h->res5.back().fused_shortcut,
                                          p.feat + (size_t)(k0 + n0) * h->res5_c, hs));
        }
        if (split) {
            VK_CHECK_HIP(hipEventRecord(ln.ev_join, h->side));
            VK_CHECK_HIP(hipStreamWaitEvent(s, ln.ev_join, 0));
        }
        if (!p.pool_part) VK_TRY(vk_mean_pool(x, kc, hh * ww, h->res5_c, p.feat + (size_t)k0 * h->res5_c, h->dt, s));
    }
    if (p.chunk >= p.K) set_stage(h, "pooled", p.pooled, h->dt, {p.K, P, P, h->res4_c});
    if (dd_chunks > 0 && dd_chunks == ceil_div(p.K, p.chunk))      // (every chunk took the dedupe path: each count has been written)
        set_stage(h, "head_windows", p.dd_u, VK_I32, {dd_chunks});    // distinct RoIPool windows per chunk
    if (tap_chunks > 0 && tap_chunks == ceil_div(p.K, p.chunk))
        set_stage(h, "head_neighbourhoods", p.nb_v, VK_I32, {tap_chunks});    // distinct nine-window neighbourhoods per chunk
    return fwd_predictor(h, p, s);
}

// The class / attribute branches of the box predictor on the p.K feature rows of p.feat (FastRCNNOutputLayers.forward
// frcnn.py:1726-1740): the one copy, behind the RoI head (fwd_head) and behind the grid pooling (vk_forward_grid_begin).
// Stages "feature_pooled", "obj_logits", "attr_logits".
static int fwd_predictor(vk_handle *h, const Plan &p, hipStream_t s) {
    const vk_config &c = h->cfg;
    set_stage(h, "feature_pooled", p.feat, VK_F32, {p.K, h->res5_c});

    const int C = c.num_classes, F = h->res5_c, E = h->emb_dim, AT = c.num_attrs;
    const int ld_cls = (C + 1 + 7) / 8 * 8, ld_attr = (AT + 1 + 7) / 8 * 8;
    VK_TRY(launch_concat_embed(p.feat, nullptr, nullptr, F, 0, p.K, p.featT, h->pdt, s));
    VK_TRY(run_conv(h, h->cls_score, p.featT, p.K, 1, 1, p.cls_logits, s, {.out_dt = VK_F32, .ldy = ld_cls}));
    VK_TRY(launch_softmax_argmax(p.cls_logits, ld_cls, p.K, C + 1, C, p.obj_prob, p.obj_cls, p.max_class, s));
    VK_TRY(launch_concat_embed(p.feat, h->emb, p.max_class, F, E, p.K, p.concat, h->pdt, s));
    VK_TRY(run_conv(h, h->fc_attr, p.concat, p.K, 1, 1, p.attr_hid, s, {.relu = true}));
    VK_TRY(run_conv(h, h->attr_score, p.attr_hid, p.K, 1, 1, p.attr_logits, s, {.out_dt = VK_F32, .ldy = ld_attr}));
    VK_TRY(launch_softmax_argmax(p.attr_logits, ld_attr, p.K, AT, AT, p.attr_prob, p.attr_cls, nullptr, s));
    set_stage(h, "obj_logits", p.cls_logits, VK_F32, {p.K, ld_cls});
    set_stage(h, "attr_logits", p.attr_logits, VK_F32, {p.K, ld_attr});
    return VK_OK;
}

// the forward's last stage event, the read-back of the non-finite flag into the ticket's pinned slot (the reference
// asserts finite boxes on the host, frcnn.py:148), the ticket's completion event.  nonfinite == nullptr: a forward that
// launched nothing (given boxes, B == 0)
static int fwd_close(vk_handle *h, const int32_t *nonfinite, hipStream_t s, int64_t *ticket) {
    if (h->timing && nonfinite) {
        VK_CHECK_HIP(hipEventRecord(h->ev[5], s));
        h->ev_valid = true;
    }
    VK_TRY(ensure_ticket_state(h));
    const int slot = (int)(h->next_ticket % vk_handle::VK_MAX_INFLIGHT);
    h->slot_stream[slot] = s;
    h->slot_caller[slot] = h->cur_caller;
    h->slot_set[slot] = nonfinite ? h->cur_set : -1;
    if (nonfinite)
        VK_CHECK_HIP(hipMemcpyAsync(&h->flag_host[slot], nonfinite, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    else
        h->flag_host[slot] = 0;     // nothing was computed (given boxes, B == 0); the slot's previous forward has ended
    VK_CHECK_HIP(hipEventRecord(h->ev_done[slot], s));
    *ticket = h->next_ticket++;
    return VK_OK;
}

// ---- the admission checks the *_begin entry points share; `who` is the entry point's prefix in the error text.  They are
// separate pieces because each entry point has its own order (the detection forward looks at the handle first, the other
// two at their arguments) ----
static int check_forward_size(const char *who, int N, int H, int W) {
    VK_REQUIRE(N >= 1 && H >= 32 && W >= 32, VK_EINVAL, "%s: bad input size N=%d H=%d W=%d", who, N, H, W);
    return VK_OK;
}

// image_shapes only bound the box clipping (frcnn.py:147-153); the reference does not check them
// against the tensor size (its own adapter passes PIL (w,h) order, adapters/frcnn.py:50-52)
static int check_image_shape(const char *who, const int32_t *image_hw, int n) {
    VK_REQUIRE(image_hw[2 * n] >= 1 && image_hw[2 * n + 1] >= 1, VK_EINVAL, "%s: image_shapes[%d]=(%d,%d) must be positive", who, n,
               image_hw[2 * n], image_hw[2 * n + 1]);
    return VK_OK;
}

static int check_forward_handle(const char *who, const vk_handle *h) {
    VK_REQUIRE(h->next_ticket - h->oldest_open < vk_handle::VK_MAX_INFLIGHT, VK_EINVAL,
               "%s_begin: %d forwards are already in flight; end the oldest first", who, vk_handle::VK_MAX_INFLIGHT);
    VK_REQUIRE(h->finalized, VK_EINVAL, "%s: vk_finalize has not been called", who);
    return VK_OK;
}

// the output arrays of a forward that writes one row per box / cell
static int check_row_outputs(const char *who, const vk_outputs *out) {
    VK_REQUIRE(out->obj_ids && out->obj_probs && out->attr_ids && out->attr_probs && out->boxes && out->preds_per_image &&
                   out->roi_features,
               VK_EINVAL, "%s: null output array", who);
    VK_REQUIRE(((uintptr_t)out->roi_features & 15) == 0, VK_EINVAL, "%s: roi_features must be 16-byte aligned", who);
    return VK_OK;
}

struct TimerScope {   // per-launch events only inside one forward
    explicit TimerScope(KernelTimer *t) { g_timer = t; }
    ~TimerScope() { g_timer = nullptr; }
};

}  // namespace vk

extern "C" {

int vk_forward_begin(vk_handle *h, const float *images_dev, int N, int H, int W, const int32_t *image_hw,
                     const float *scales_yx, const vk_roi_params *rp, const vk_outputs *out, void *stream, int64_t *ticket) {
    return vk_forward_begin_ignorey(h, images_dev, N, H, W, image_hw, scales_yx, rp, out, stream, ticket, nullptr);
}

// Shared by the two all-class selections (after fwd_head).  bbox_pred in the packed form of the linear path, once per handle
// (dense 1x1: row-major rows, zero rows up to a whole tile).
static int ensure_bbox_lin(vk_handle *h, int nrow, int F, hipStream_t s) {
    if (h->bbox_lin_w) return VK_OK;
    const int cp = vk_packed_cout(nrow);
    if (cp == nrow) {
        h->bbox_lin_w = h->bbox_w;
        h->bbox_lin_b = h->bbox_b;
        return VK_OK;
    }
    const size_t row = (size_t)F * dtype_size(h->pdt);
    void *w = nullptr, *b = nullptr;
    VK_TRY(dev_alloc(h, (size_t)cp * row, &w));
    VK_TRY(dev_alloc(h, (size_t)cp * sizeof(float), &b));
    VK_CHECK_HIP(hipMemsetAsync(w, 0, (size_t)cp * row, s));
    VK_CHECK_HIP(hipMemsetAsync(b, 0, (size_t)cp * sizeof(float), s));
    VK_CHECK_HIP(hipMemcpyAsync(w, h->bbox_w, (size_t)nrow * row, hipMemcpyDeviceToDevice, s));
    VK_CHECK_HIP(hipMemcpyAsync(b, h->bbox_b, (size_t)nrow * sizeof(float), hipMemcpyDeviceToDevice, s));
    VK_CHECK_HIP(hipStreamSynchronize(s));      // once per handle: the next forward may read them from another stream
    h->bbox_lin_w = w;
    h->bbox_lin_b = (const float *)b;
    return VK_OK;
}

// soft-max of every class and bbox_pred over all its rows through the linear path: stages "obj_scores", "box_deltas", "attr_prob"
static int class_scores_and_deltas(vk_handle *h, const Plan &p, float *scores, int ld_cls, float *deltas, int ld_box, int nrow,
                                   hipStream_t s) {
    const int C = h->cfg.num_classes, F = h->res5_c, K = p.K;
    VK_TRY(launch_class_probs(p.cls_logits, ld_cls, K, C + 1, scores, ld_cls, s));
    ConvArgs g;
    fill_conv_args(g, 1, 1, K, F, nrow, ld_box, 1, 1, 0, 1, 1, 0, h->pdt, VK_F32);
    g.x = p.featT;
    g.w = h->bbox_lin_w;
    g.bias = h->bbox_lin_b;
    g.y = deltas;
    VK_TRY(launch_conv(g, s));
    set_stage(h, "obj_scores", scores, VK_F32, {K, ld_cls});
    set_stage(h, "box_deltas", deltas, VK_F32, {K, ld_box});
    set_stage(h, "attr_prob", p.attr_prob, VK_F32, {K});
    if (h->timing) VK_CHECK_HIP(hipEventRecord(h->ev[4], s));
    return VK_OK;
}

// What the two all-class selections do before their own kernel: bbox_pred in the linear form, the selection's arena grown to
// [scores | deltas | extra_bytes of the caller's own] (256-byte aligned pieces, in that order), the scores and deltas computed
// into it, and `a` built on them (fill_per_class_args).  *extra is where the caller's bytes start.
static int select_open(vk_handle *h, const Plan &p, const vk_select_params *sp, const float *scales_dev, const vk_outputs *out,
                       char **arena, size_t *arena_bytes, size_t extra_bytes, hipStream_t s, PerClassArgs &a, char **extra) {
    const vk_config &c = h->cfg;
    const int C = c.num_classes, F = h->res5_c, K = p.K;
    const int nrow = 4 * (c.cls_agnostic_bbox_reg ? 1 : C);
    const int ld_cls = (C + 1 + 7) / 8 * 8, ld_box = (nrow + 7) / 8 * 8;
    VK_TRY(ensure_bbox_lin(h, nrow, F, s));
    Carver cv(nullptr);
    const size_t o_scores = cv.off;
    cv.take((size_t)K * ld_cls * sizeof(float));
    const size_t o_deltas = cv.off;
    cv.take((size_t)K * ld_box * sizeof(float));
    const size_t o_extra = cv.off;
    VK_TRY(grow_device_block(arena, arena_bytes, o_extra + extra_bytes, false));
    float *scores = (float *)(*arena + o_scores), *deltas = (float *)(*arena + o_deltas);
    *extra = *arena + o_extra;
    VK_TRY(class_scores_and_deltas(h, p, scores, ld_cls, deltas, ld_box, nrow, s));
    fill_per_class_args(a, scores, ld_cls, deltas, ld_box, c.cls_agnostic_bbox_reg, p.prop_boxes, p.prop_counts, p.feat, p.attr_prob,
                        p.attr_cls, F, p.R, C, p.image_hw, scales_dev, c.roi_bbox_weights, sp, out, p.keep_ids, p.nonfinite);
    return VK_OK;
}

// The per-class end of a detection forward (after fwd_head): soft-max of every class, bbox_pred over all its rows through the
// linear path, per-class NMS + finalize (per_class.hip).  Stages "obj_scores", "box_deltas", "max_conf", "keep_ids".
static int fwd_per_class(vk_handle *h, const Plan &p, const vk_select_params *sp, const float *scales_dev, const vk_outputs *out,
                         hipStream_t s) {
    Carver own(nullptr);
    const size_t o_best = own.off;
    own.take((size_t)p.K * sizeof(unsigned long long));
    const size_t o_conf = own.off;
    own.take((size_t)p.K * sizeof(float));
    vk_handle::WorkSet &ws = h->sets[h->cur_set];
    PerClassArgs a;
    char *mine = nullptr;
    VK_TRY(select_open(h, p, sp, scales_dev, out, &ws.pc_arena, &ws.pc_arena_bytes, own.off, s, a, &mine));
    a.best = (unsigned long long *)(mine + o_best);
    a.max_conf = (float *)(mine + o_conf);
    VK_TRY(launch_per_class_select(a, p.N, s));
    set_stage(h, "max_conf", a.max_conf, VK_F32, {p.N, p.R});
    set_stage(h, "keep_ids", p.keep_ids, VK_I64, {p.N, sp->roi.max_detections});
    return VK_OK;
}

// The detector-style end of a detection forward: the same scores and all-class deltas, then
// detections.hip.  Stages "obj_scores", "box_deltas", "attr_prob", "keep_ids", "n_survivors".
static int fwd_detections(vk_handle *h, const Plan &p, const vk_select_params *sp, const float *scales_dev, const vk_outputs *out,
                          hipStream_t s) {
    const int C = h->cfg.num_classes;
    VK_REQUIRE(p.N <= 65535 && p.R <= 1024 && C < (1 << 20), VK_EINVAL, "forward: the detections selection takes N=%d <= 65535, "
               "R=%d <= 1024, C=%d < 2^20", p.N, p.R, C);
    Carver own(nullptr);
    const size_t o_nsurv = own.off;
    own.take((size_t)p.N * sizeof(int32_t));
    const size_t o_work = own.off;
    own.take(det_workspace_bytes(p.N, p.R, C));
    vk_handle::WorkSet &ws = h->sets[h->cur_set];
    DetArgs d;
    memset(&d, 0, sizeof(d));
    char *mine = nullptr;
    VK_TRY(select_open(h, p, sp, scales_dev, out, &ws.det_arena, &ws.det_arena_bytes, own.off, s, d.pc, &mine));
    det_carve(d, mine + o_work, p.N, p.R, C);
    d.n_survivors = (int32_t *)(mine + o_nsurv);
    VK_TRY(launch_detections_select(d, p.N, s));
    set_stage(h, "keep_ids", p.keep_ids, VK_I64, {p.N, sp->roi.max_detections});
    set_stage(h, "n_survivors", d.n_survivors, VK_I32, {p.N});
    return VK_OK;
}

// vk_forward_begin_ignorey / vk_forward_begin_select: sel == nullptr is the class-max mode on rp, else rp == &sel->roi and
// sel->mode is VK_SELECT_PER_CLASS or VK_SELECT_DETECTIONS
static int forward_detect(vk_handle *h, const float *images_dev, int N, int H, int W, const int32_t *image_hw,
                          const float *scales_yx, const vk_roi_params *rp, const vk_select_params *sel, const vk_outputs *out,
                          void *stream, int64_t *ticket, const vk_ignorey *ignorey);

int vk_forward_begin_ignorey(vk_handle *h, const float *images_dev, int N, int H, int W, const int32_t *image_hw,
                             const float *scales_yx, const vk_roi_params *rp, const vk_outputs *out, void *stream, int64_t *ticket,
                             const vk_ignorey *ignorey) {
    return forward_detect(h, images_dev, N, H, W, image_hw, scales_yx, rp, nullptr, out, stream, ticket, ignorey);
}

int vk_forward_begin_select(vk_handle *h, const float *images_dev, int N, int H, int W, const int32_t *image_hw,
                            const float *scales_yx, const vk_select_params *sp, const vk_outputs *out, void *stream, int64_t *ticket,
                            const vk_ignorey *ignorey) {
    VK_REQUIRE(sp, VK_EINVAL, "forward: null argument");
    VK_REQUIRE(sp->mode == VK_SELECT_CLASS_MAX || sp->mode == VK_SELECT_PER_CLASS || sp->mode == VK_SELECT_DETECTIONS, VK_EINVAL,
               "forward: unknown selection mode %d", sp->mode);
    if (sp->mode == VK_SELECT_PER_CLASS) VK_TRY(check_select_params(sp, "forward"));
    if (sp->mode == VK_SELECT_DETECTIONS) VK_TRY(check_detections_params(sp, "forward"));
    return forward_detect(h, images_dev, N, H, W, image_hw, scales_yx, &sp->roi, sp->mode == VK_SELECT_CLASS_MAX ? nullptr : sp, out,
                          stream, ticket, ignorey);
}

static int forward_detect(vk_handle *h, const float *images_dev, int N, int H, int W, const int32_t *image_hw,
                          const float *scales_yx, const vk_roi_params *rp, const vk_select_params *sel, const vk_outputs *out,
                          void *stream, int64_t *ticket, const vk_ignorey *ignorey) {
    VK_REQUIRE(h && images_dev && image_hw && rp && out && ticket, VK_EINVAL, "forward: null argument");
    // the reference filters by the bands only when scales_yx is given too (frcnn.py:328); no bands == the plain launch sequence
    const vk_ignorey *ig = scales_yx && ignorey && ignorey->max_per_image > 0 ? ignorey : nullptr;
    if (ig) {
        VK_REQUIRE(ig->max_per_image <= VK_MAX_IGNOREY, VK_EINVAL, "ignorey: max_per_image=%d must be in 0..%d", ig->max_per_image,
                   VK_MAX_IGNOREY);
        VK_REQUIRE(ig->bands && ig->counts, VK_EINVAL, "ignorey: null bands / counts");
        VK_REQUIRE(ig->f64 == 0 || ig->f64 == 1, VK_EINVAL, "ignorey: f64=%d must be 0 or 1", ig->f64);
        for (int n = 0; n < N; ++n) {
            const int J = ig->counts[n];
            VK_REQUIRE(J >= 0 && J <= ig->max_per_image, VK_EINVAL, "ignorey: counts[%d]=%d must be in 0..%d", n, J, ig->max_per_image);
            for (int k = 0; k < 2 * J; ++k) {
                const size_t at = ((size_t)n * ig->max_per_image) * 2 + k;
                const double v = ig->f64 ? static_cast<const double *>(ig->bands)[at] : (double)static_cast<const float *>(ig->bands)[at];
                // int() of the band (frcnn.py:365-366) raises on these in the reference
                VK_REQUIRE(std::isfinite(v) && std::fabs(v) < 2147483648.0, VK_EINVAL, "ignorey: image %d band %d holds %g (must be finite, "
                           "|value| < 2^31)", n, k / 2, v);
            }
        }
    }
    VK_TRY(check_forward_handle("forward", h));
    VK_TRY(check_forward_size("forward", N, H, W));
    VK_REQUIRE(rp->num_nms_thresh >= 1 && rp->num_nms_thresh <= VK_MAX_NMS_THRESH, VK_EINVAL, "forward: 1..%d nms thresholds", VK_MAX_NMS_THRESH);
    if (sel && sel->mode == VK_SELECT_DETECTIONS)       // a proposal may come out under several classes (check_detections_params)
        VK_REQUIRE(N <= 65535, VK_EINVAL, "forward: the detections selection takes at most 65535 images, got N=%d", N);
    else
        VK_REQUIRE(rp->max_detections >= 1 && rp->max_detections <= h->cfg.post_nms_topk, VK_EINVAL,
                   "forward: max_detections=%d must be in 1..POST_NMS_TOPK_TEST", rp->max_detections);
    for (int n = 0; n < N; ++n) VK_TRY(check_image_shape("forward", image_hw, n));
    VK_CHECK_HIP(hipSetDevice(h->device));
    hipStream_t s = nullptr;            // the forward's stream: the caller's, or the ticket's lane (fwd_route)
    const vk_config &c = h->cfg;
    const int D = rp->max_detections;
    TimerScope timer_scope(h->ktimer);
    const bool tm = h->timing;

    Plan p;
    VK_TRY(fwd_open(h, N, H, W, c.post_nms_topk, D, image_hw, scales_yx, nullptr, ig, (hipStream_t)stream, &p, &s));
    const void *res4 = nullptr;
    VK_TRY(fwd_backbone(h, p, images_dev, s, &res4));

    // ---- RPN head (RPNHead.forward frcnn.py:1561-1572) ----
    const int ld_rpn = (5 * h->A + 7) / 8 * 8;
    VK_TRY(run_conv(h, h->rpn_conv, res4, N, p.Hf, p.Wf, p.rpn_hid, s, {.relu = true}));
    VK_TRY(run_conv(h, h->rpn_heads, p.rpn_hid, N, p.Hf, p.Wf, p.rpn_out, s, {.out_dt = VK_F32, .ldy = ld_rpn}));
    set_stage(h, "rpn_out", p.rpn_out, VK_F32, {N, p.Hf, p.Wf, ld_rpn});
    if (tm) VK_CHECK_HIP(hipEventRecord(h->ev[2], s));

    // ---- proposals (RPN.inference frcnn.py:1615-1638) ----
    vk_ignorey ig_dev{};
    if (ig) {
        ig_dev.bands = p.bands;
        ig_dev.counts = p.band_counts;
        ig_dev.max_per_image = ig->max_per_image;
        ig_dev.f64 = ig->f64;
    }
    VK_TRY(vk_rpn_proposals_ignorey(p.rpn_out, ld_rpn, p.rpn_out + h->A, ld_rpn, N, p.Hf, p.Wf, h->A, h->cell_anchors, 16,
                                    c.anchor_offset, p.image_hw, c.rpn_bbox_weights, c.rpn_min_size, c.rpn_nms_thresh,
                                    c.pre_nms_topk, c.post_nms_topk, p.prop_boxes, p.prop_logits, p.prop_counts, p.nonfinite,
                                    p.rpn_ws, p.rpn_ws_bytes, s, ig ? &ig_dev : nullptr));
    VK_TRY(launch_make_rois(p.prop_boxes, N, p.R, p.rois, s));
    set_stage(h, "proposal_boxes", p.prop_boxes, VK_F32, {N, p.R, 4});
    set_stage(h, "proposal_logits", p.prop_logits, VK_F32, {N, p.R});
    set_stage(h, "proposal_counts", p.prop_counts, VK_I32, {N});
    if (tm) VK_CHECK_HIP(hipEventRecord(h->ev[3], s));

    // ---- RoI heads + box predictor; the arg-max class's box regression ----
    VK_TRY(fwd_head(h, p, res4, s));
    if (sel) {                 // every class's box regression, NMS per class: one output per proposal, or a detector's triples
        if (sel->mode == VK_SELECT_DETECTIONS)
            VK_TRY(fwd_detections(h, p, sel, scales_yx ? p.scales : nullptr, out, s));
        else
            VK_TRY(fwd_per_class(h, p, sel, scales_yx ? p.scales : nullptr, out, s));
        return fwd_close(h, p.nonfinite, s, ticket);
    }
    const int F = h->res5_c;
    VK_TRY(launch_chosen_deltas(p.featT, F, h->bbox_w, h->bbox_b, p.obj_cls, c.cls_agnostic_bbox_reg, F, p.K, p.chosen, h->pdt, s));
    set_stage(h, "chosen_deltas", p.chosen, VK_F32, {p.K, 4});
    if (tm) VK_CHECK_HIP(hipEventRecord(h->ev[4], s));

    // ---- outputs (ROIOutputs.inference frcnn.py:1262-1294) ----
    RoiFinalArgs a;
    fill_roi_final_args(a, p.obj_prob, p.obj_cls, p.attr_prob, p.attr_cls, p.chosen, 4, 1, p.prop_boxes, p.prop_counts, p.feat, F, p.R,
                        p.image_hw, scales_yx ? p.scales : nullptr, c.roi_bbox_weights, rp, out, p.keep_ids, p.nonfinite);
    VK_TRY(launch_roi_final(a, N, s));
    set_stage(h, "keep_ids", p.keep_ids, VK_I64, {N, D});
    return fwd_close(h, p.nonfinite, s, ticket);
}

int vk_forward_boxes_begin(vk_handle *h, const float *images_dev, int N, int H, int W, const int32_t *image_hw,
                           const float *scales_yx, const float *boxes_dev, int B, const int32_t *counts, const vk_outputs *out,
                           void *stream, int64_t *ticket) {
    // the arguments first, then the handle: every check here runs before anything touches the device
    VK_REQUIRE(images_dev && image_hw && counts && out && ticket, VK_EINVAL, "forward_boxes: null argument");
    VK_TRY(check_forward_size("forward_boxes", N, H, W));
    VK_REQUIRE(B >= 0 && B <= 1024, VK_EINVAL, "forward_boxes: B=%d boxes per image must be in 0..1024", B);
    VK_REQUIRE(B == 0 || boxes_dev, VK_EINVAL, "forward_boxes: null boxes with B=%d", B);
    VK_REQUIRE(out->preds_per_image, VK_EINVAL, "forward_boxes: null preds_per_image");
    if (B > 0) VK_TRY(check_row_outputs("forward_boxes", out));       // (B == 0 writes preds_per_image alone)
    for (int n = 0; n < N; ++n) {
        VK_REQUIRE(counts[n] >= 0 && counts[n] <= B, VK_EINVAL, "forward_boxes: counts[%d]=%d must be in 0..B=%d", n, counts[n], B);
        VK_TRY(check_image_shape("forward_boxes", image_hw, n));
    }
    VK_REQUIRE(h, VK_EINVAL, "forward_boxes: null handle");
    VK_TRY(check_forward_handle("forward_boxes", h));
    VK_CHECK_HIP(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (B == 0) {       // every image is empty: a zero-detection block, no kernel, no stage events; on the caller's stream, no working set
        h->stages_out.clear();
        h->pooled_expand.pending = false;
        h->ev_valid = false;
        h->cur_caller = s;
        VK_CHECK_HIP(hipMemsetAsync(out->preds_per_image, 0, sizeof(int64_t) * (size_t)N, s));
        return fwd_close(h, nullptr, s, ticket);
    }
    TimerScope timer_scope(h->ktimer);
    const bool tm = h->timing;

    Plan p;
    VK_TRY(fwd_open(h, N, H, W, B, B, image_hw, scales_yx, counts, nullptr, (hipStream_t)stream, &p, &s));
    const void *res4 = nullptr;
    VK_TRY(fwd_backbone(h, p, images_dev, s, &res4));
    if (tm) VK_CHECK_HIP(hipEventRecord(h->ev[2], s));          // no RPN head

    // ---- the caller's boxes in place of the proposals: scale, finite check, _clip_box (frcnn.py:147-153), RoI rows ----
    VK_TRY(launch_given_boxes_ingest(boxes_dev, p.prop_counts, p.image_hw, scales_yx ? p.scales : nullptr, N, B, p.prop_boxes,
                                     p.rois, p.nonfinite, s));
    set_stage(h, "proposal_boxes", p.prop_boxes, VK_F32, {N, B, 4});
    set_stage(h, "proposal_counts", p.prop_counts, VK_I32, {N});
    if (tm) VK_CHECK_HIP(hipEventRecord(h->ev[3], s));

    VK_TRY(fwd_head(h, p, res4, s));
    if (tm) VK_CHECK_HIP(hipEventRecord(h->ev[4], s));

    // ---- outputs: every box in input order, no regression, no NMS ----
    VK_TRY(launch_given_box_outputs(p.obj_prob, p.obj_cls, p.attr_prob, p.attr_cls, p.prop_boxes, p.prop_counts,
                                    scales_yx ? p.scales : nullptr, p.feat, h->res5_c, N, B, *out, s));
    return fwd_close(h, p.nonfinite, s, ticket);
}

int vk_forward_grid_begin(vk_handle *h, const float *images_dev, int N, int H, int W, const int32_t *image_hw,
                          const float *scales_yx, int Gh, int Gw, const vk_outputs *out, void *stream, int64_t *ticket) {
    // the arguments first, then the handle: every check here runs before anything touches the device
    VK_REQUIRE(images_dev && image_hw && out && ticket, VK_EINVAL, "forward_grid: null argument");
    VK_TRY(check_forward_size("forward_grid", N, H, W));
    VK_REQUIRE(Gh >= 1 && Gw >= 1 && (long)Gh * Gw <= 1024, VK_EINVAL, "forward_grid: grid (%d, %d) must have 1..1024 cells", Gh, Gw);
    VK_TRY(check_row_outputs("forward_grid", out));
    for (int n = 0; n < N; ++n) VK_TRY(check_image_shape("forward_grid", image_hw, n));
    VK_REQUIRE(h, VK_EINVAL, "forward_grid: null handle");
    VK_TRY(check_forward_handle("forward_grid", h));
    const int G = Gh * Gw;
    // the working set this forward will get must hold the whole map in each head buffer: refuse before anything is enqueued
    const Plan need = make_plan(h, nullptr, N, H, W, G, G, true);
    const size_t map_rows = (size_t)N * need.Hf * need.Wf;
    VK_REQUIRE(need.head_rows >= map_rows, VK_EINVAL, "forward_grid: the working set holds %zu Res5 rows, the %d x %d x %d map needs %zu",
               need.head_rows, N, need.Hf, need.Wf, map_rows);
    VK_CHECK_HIP(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    TimerScope timer_scope(h->ktimer);
    const bool tm = h->timing;

    Plan p;
    std::vector<int32_t> counts((size_t)N, G);          // every cell is a row: fwd_open copies them into the ticket's slot
    VK_TRY(fwd_open(h, N, H, W, G, G, image_hw, scales_yx, counts.data(), nullptr, (hipStream_t)stream, &p, &s, true));
    VK_REQUIRE(p.head_rows >= map_rows, VK_EINVAL, "internal: grid plan of %zu rows for a map of %zu", p.head_rows, map_rows);
    const void *res4 = nullptr;
    VK_TRY(fwd_backbone(h, p, images_dev, s, &res4));
    if (tm) {                                            // no RPN head, no proposals
        VK_CHECK_HIP(hipEventRecord(h->ev[2], s));
        VK_CHECK_HIP(hipEventRecord(h->ev[3], s));
    }

    // ---- Res5 over the whole map (roi_heads.res5 on res4, frcnn.py:1344-1355): one launch per layer, no chunks ----
    // Each block's output stays in a buffer of its own (stages "grid_res5_<b>", the last one "grid_map"): h_sc is free from
    // block 1 on, because only block 0 has a projection shortcut.
    const void *x = res4;
    void *outs[3] = {p.h_a, p.h_b, p.h_sc};
    int hh = p.Hf, ww = p.Wf;
    for (size_t bi = 0; bi < h->res5.size(); ++bi) {
        int ho, wo;
        void *y = outs[bi % 3];
        VK_TRY(run_block(h, h->res5[bi], x, N, hh, ww, p.h_t1, p.h_t2, p.h_sc, y, s, &ho, &wo));
        hh = ho;
        ww = wo;
        x = y;
        if (bi + 1 < h->res5.size() && bi < 2) set_stage(h, bi == 0 ? "grid_res5_0" : "grid_res5_1", y, h->dt, {N, hh, ww, h->res5_c});
    }
    VK_REQUIRE((size_t)N * hh * ww <= map_rows, VK_EINVAL, "internal: Res5 map %dx%d is larger than res4's %dx%d", hh, ww, p.Hf, p.Wf);
    set_stage(h, "grid_map", x, h->dt, {N, hh, ww, h->res5_c});

    // ---- the cells: fp64 average per cell and channel, the cell boxes in network pixels (scaled by the output kernel) ----
    const int S = h->cfg.res5_halve ? 32 : 16;          // res4's stride, doubled by block 0's under RES5HALVE
    VK_TRY(vk_grid_pool(x, N, hh, ww, h->res5_c, h->dt, p.image_hw, nullptr, S, Gh, Gw, p.feat, h->res5_c, p.prop_boxes, s));
    set_stage(h, "proposal_boxes", p.prop_boxes, VK_F32, {N, G, 4});
    VK_TRY(fwd_predictor(h, p, s));
    if (tm) VK_CHECK_HIP(hipEventRecord(h->ev[4], s));

    // ---- outputs: every cell in row-major order, counts all G ----
    VK_TRY(launch_given_box_outputs(p.obj_prob, p.obj_cls, p.attr_prob, p.attr_cls, p.prop_boxes, p.prop_counts,
                                    scales_yx ? p.scales : nullptr, p.feat, h->res5_c, N, G, *out, s));
    return fwd_close(h, p.nonfinite, s, ticket);
}

int vk_forward_end(vk_handle *h, int64_t ticket) {
    VK_REQUIRE(h, VK_EINVAL, "forward_end: null handle");
    VK_REQUIRE(ticket == h->oldest_open && ticket < h->next_ticket, VK_EINVAL,
               "forward_end: ticket %lld is not the oldest forward in flight (%lld)", (long long)ticket, (long long)h->oldest_open);
    const int slot = (int)(ticket % vk_handle::VK_MAX_INFLIGHT);
    h->oldest_open++;
    VK_CHECK_HIP(hipSetDevice(h->device));
    // a forward that ran on a lane's stream: whatever the caller enqueues next on its own stream sees the outputs
    if (h->slot_stream[slot] != h->slot_caller[slot]) VK_CHECK_HIP(hipStreamWaitEvent(h->slot_caller[slot], h->ev_done[slot], 0));
    VK_CHECK_HIP(hipEventSynchronize(h->ev_done[slot]));
    if (h->ktimer) h->ktimer->collect();
    VK_REQUIRE(h->flag_host[slot] == 0, VK_ENONFINITE, "Box tensor contains infinite or NaN!");
    return VK_OK;
}

int vk_enable_kernel_timing(vk_handle *h, int enable) {
    VK_REQUIRE(h, VK_EINVAL, "null handle");
    if (enable && !h->ktimer) h->ktimer = new KernelTimer();
    if (!enable && h->ktimer) {
        delete h->ktimer;
        h->ktimer = nullptr;
    }
    return VK_OK;
}

int vk_get_kernel_timing(vk_handle *h, int64_t *launches, double *ms, double *flops, double *bytes, int reset) {
    VK_REQUIRE(h && launches && ms && flops && bytes, VK_EINVAL, "null argument");
    VK_REQUIRE(h->ktimer, VK_EINVAL, "kernel timing is not enabled");
    for (int i = 0; i < VK_NUM_KERNEL_BUCKETS; ++i) {
        launches[i] = h->ktimer->launches[i];
        ms[i] = h->ktimer->ms[i];
        flops[i] = h->ktimer->flops[i];
        bytes[i] = h->ktimer->bytes[i];
        if (reset) {
            h->ktimer->bytes[i] = 0;
            h->ktimer->launches[i] = 0;
            h->ktimer->ms[i] = 0;
            h->ktimer->flops[i] = 0;
        }
    }
    return VK_OK;
}

}  // extern "C"
