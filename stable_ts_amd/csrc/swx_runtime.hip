// swx_runtime.hip -- the model handle of libswx.so's C ABI (include/swx.h): weight arena, workspace, profiler and A/B switches,
// and the host-side drivers of the spectrogram, the encoder and the cross-K/V projection.  The decoder forward pass is in
// swx_decoder.hip, the decoding loop in swx_decjob.hip, the teacher-forced passes in swx_score.hip, the test hooks in swx_testhooks.hip.
// No device allocation happens here: the caller binds the arena and the workspace (PyTorch owns the memory).
#include <cmath>
#include <cstring>
#include <cstdio>
#include "swx_model.h"

namespace {

size_t add_slot(swx_model *m, size_t &cur, const std::string &name, int kind, int64_t rows, int64_t cols, int64_t dst_ld,
                size_t bytes, size_t base_off = (size_t)-1, size_t sub_off = 0)
{
    Slot s;
    s.kind = kind; s.rows = rows; s.cols = cols; s.dst_ld = dst_ld;
    if (base_off == (size_t)-1) { s.off = cur; cur = align_up(cur + bytes); }
    else s.off = base_off + sub_off;
    m->slots[name] = s;
    return s.off;
}

void build_layout(swx_model *m)
{
    const swx_dims &D = m->dims;
    const size_t e = m->esz;
    size_t cur = 0;
    auto mat = [&](const std::string &n, int64_t r, int64_t c) { return add_slot(m, cur, n, SK_MAT, r, c, c, (size_t)r * c * e); };
    auto vec = [&](const std::string &n, int64_t c) { return add_slot(m, cur, n, SK_VEC, 1, c, c, (size_t)c * 4); };
    auto reserve = [&](size_t bytes) { size_t o = cur; cur = align_up(cur + bytes); return o; };

    const int da = D.n_audio_state, dt = D.n_text_state;
    m->Cp = (D.n_mels + 31) / 32 * 32;
    m->o_conv1_w = add_slot(m, cur, "encoder.conv1.weight", SK_CONV, da, D.n_mels, m->Cp, (size_t)da * 3 * m->Cp * e);
    m->o_conv1_b = vec("encoder.conv1.bias", da);
    m->o_conv2_w = add_slot(m, cur, "encoder.conv2.weight", SK_CONV, da, da, da, (size_t)da * 3 * da * e);
    m->o_conv2_b = vec("encoder.conv2.bias", da);
    m->o_enc_pos = add_slot(m, cur, "encoder.positional_embedding", SK_VEC, 1, (int64_t)D.n_audio_ctx * da, 0, (size_t)D.n_audio_ctx * da * 4);

    auto block = [&](const std::string &p, int d, bool cross) {
        LayerW w{};
        w.ln1_g = vec(p + "attn_ln.weight", d);
        w.ln1_b = vec(p + "attn_ln.bias", d);
        w.wqkv = reserve((size_t)3 * d * d * e);
        add_slot(m, cur, p + "attn.query.weight", SK_MAT, d, d, d, 0, w.wqkv, 0);
        add_slot(m, cur, p + "attn.key.weight", SK_MAT, d, d, d, 0, w.wqkv, (size_t)d * d * e);
        add_slot(m, cur, p + "attn.value.weight", SK_MAT, d, d, d, 0, w.wqkv, (size_t)2 * d * d * e);
        w.bqkv = reserve((size_t)3 * d * 4);
        add_slot(m, cur, p + "attn.query.bias", SK_VEC, 1, d, d, 0, w.bqkv, 0);
        add_slot(m, cur, p + "attn.value.bias", SK_VEC, 1, d, d, 0, w.bqkv, (size_t)2 * d * 4);
        w.wo = mat(p + "attn.out.weight", d, d);
        w.bo = vec(p + "attn.out.bias", d);
        if (cross) {
            w.lnx_g = vec(p + "cross_attn_ln.weight", d);
            w.lnx_b = vec(p + "cross_attn_ln.bias", d);
            w.wcq = mat(p + "cross_attn.query.weight", d, d);
            w.bcq = vec(p + "cross_attn.query.bias", d);
            w.wckv = reserve((size_t)2 * d * d * e);
            add_slot(m, cur, p + "cross_attn.key.weight", SK_MAT, d, d, d, 0, w.wckv, 0);
            add_slot(m, cur, p + "cross_attn.value.weight", SK_MAT, d, d, d, 0, w.wckv, (size_t)d * d * e);
            w.bckv = reserve((size_t)2 * d * 4);
            add_slot(m, cur, p + "cross_attn.value.bias", SK_VEC, 1, d, d, 0, w.bckv, (size_t)d * 4);
            w.wco = mat(p + "cross_attn.out.weight", d, d);
            w.bco = vec(p + "cross_attn.out.bias", d);
        }
        w.ln2_g = vec(p + "mlp_ln.weight", d);
        w.ln2_b = vec(p + "mlp_ln.bias", d);
        w.w1 = mat(p + "mlp.0.weight", 4 * d, d);
        w.b1 = vec(p + "mlp.0.bias", 4 * d);
        w.w2 = mat(p + "mlp.2.weight", d, 4 * d);
        w.b2 = vec(p + "mlp.2.bias", d);
        return w;
    };
    for (int l = 0; l < D.n_audio_layer; ++l) m->enc.push_back(block("encoder.blocks." + std::to_string(l) + ".", da, false));
    m->o_lnpost_g = vec("encoder.ln_post.weight", da);
    m->o_lnpost_b = vec("encoder.ln_post.bias", da);
    m->o_tok_emb = mat("decoder.token_embedding.weight", D.n_vocab, dt);
    m->o_dec_pos = add_slot(m, cur, "decoder.positional_embedding", SK_VEC, 1, (int64_t)D.n_text_ctx * dt, 0, (size_t)D.n_text_ctx * dt * 4);
    for (int l = 0; l < D.n_text_layer; ++l) m->dec.push_back(block("decoder.blocks." + std::to_string(l) + ".", dt, true));
    {
        int mt = 0, ks = 0;
        m->has_fold = m->dtype == SWX_F16 && swx_dec_plan(64, 3 * dt, dt, DEC_LN, &mt, &ks) == 0 &&
                      swx_dec_plan(64, dt, 4 * dt, DEC_RES | DEC_SLAB, &mt, &ks) == 0;
        if (m->has_fold)
            for (auto &w : m->dec) {
                w.wqkv_f = reserve((size_t)3 * dt * dt * e); w.qkv_c1 = reserve((size_t)3 * dt * 4); w.qkv_c2 = reserve((size_t)3 * dt * 4);
                w.wcq_f = reserve((size_t)dt * dt * e); w.cq_c1 = reserve((size_t)dt * 4); w.cq_c2 = reserve((size_t)dt * 4);
                w.w1_f = reserve((size_t)4 * dt * dt * e); w.w1_c1 = reserve((size_t)4 * dt * 4); w.w1_c2 = reserve((size_t)4 * dt * 4);
                w.wo_p = reserve((size_t)dt * dt * e); w.wco_p = reserve((size_t)dt * dt * e); w.w2_p = reserve((size_t)4 * dt * dt * e);
            }
    }
    m->o_ln_g = vec("decoder.ln.weight", dt);
    m->o_ln_b = vec("decoder.ln.bias", dt);
    // constants
    m->o_hann = vec("const.hann", SWX_N_FFT);
    m->o_filters = add_slot(m, cur, "const.mel_filters", SK_VEC, 1, (int64_t)D.n_mels * 201, 0, (size_t)D.n_mels * 201 * 4);
    m->o_twiddle = reserve(sizeof(double2) * SWX_N_FFT);
    m->o_heads = reserve(sizeof(int32_t) * (size_t)D.n_text_layer * D.n_text_head);
    m->o_zeros = reserve(256);
    m->arena_bytes = cur;
}

void default_alignment_heads(swx_model *m)
{
    const swx_dims &D = m->dims;
    m->heads_by_layer.assign(D.n_text_layer, {});
    for (int l = D.n_text_layer / 2; l < D.n_text_layer; ++l)
        for (int h = 0; h < D.n_text_head; ++h) m->heads_by_layer[l].push_back(h);
}

int upload_heads(swx_model *m)
{
    const swx_dims &D = m->dims;
    std::vector<int32_t> flat;
    m->head_slot0.assign(D.n_text_layer, 0);
    for (int l = 0; l < D.n_text_layer; ++l) {
        m->head_slot0[l] = (int)flat.size();
        for (int h : m->heads_by_layer[l]) flat.push_back(h);
    }
    m->n_align = (int)flat.size();
    m->heads_flat = flat;
    // same count as the bound workspace was laid out for: refresh its copy in place; a different count needs a re-bind
    // (swx_score / swx_score_qk refuse to run until then), which uploads the list
    if (m->ws && m->n_align == m->ws_n_align && !flat.empty()) {
        hipError_t e = hipMemcpy(m->ws + m->L.heads, flat.data(), flat.size() * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) return -100 - (int)e;
    }
    return 0;
}

void ws_layout(const swx_model *m, int Bmax, int Mmax, int n_align, swx_model::WsLayout &L)
{
    const swx_dims &D = m->dims;
    const size_t e = m->esz;
    const int da = D.n_audio_state, dt = D.n_text_state;
    const int dmax = da > dt ? da : dt;
    const int TS = D.n_text_ctx + 1;
    size_t cur = 0;
    auto take = [&](size_t bytes) { size_t o = cur; cur = align_up(cur + bytes); return o; };
    int64_t rows_big = (int64_t)Bmax * D.n_audio_ctx;
    if ((int64_t)Bmax * D.n_text_ctx > rows_big) rows_big = (int64_t)Bmax * D.n_text_ctx;
    if (Mmax > rows_big) rows_big = Mmax;
    L.rows_big = rows_big;
    L.melT = take((size_t)Bmax * 3002 * m->Cp * e);
    L.h1 = take((size_t)Bmax * 3002 * da * e);
    L.x = take((size_t)rows_big * dmax * e);
    L.h = take((size_t)rows_big * dmax * e);
    L.qkv = take((size_t)rows_big * 3 * dmax * e);
    L.att = take((size_t)rows_big * dmax * e);
    L.u = take((size_t)rows_big * 4 * dmax * e);
    L.gmax = take((size_t)Bmax * 4);
    L.small_i32 = take((size_t)SMALL_I32 * 4);
    L.zeros_i32 = take((size_t)(Mmax > Bmax ? Mmax : Bmax) * 4 + 256);
    L.ticket = take((size_t)SWX_DEC_TICKETS * 4);       // arrival counters of the in-launch slab reduction (zero between launches)
    swx_decode_state_layout(take, Bmax, Mmax, TS, D.n_text_ctx, (size_t)Bmax * 3, L.dec);
    int64_t lrows = (int64_t)Mmax + 2 * Bmax;     // M step rows + the 2W prefill rows parked at the tail
    if (lrows < 64) lrows = 64;
    L.logits_rows = lrows;
    L.logits = take((size_t)lrows * D.n_vocab * 4);
    L.hid2 = take((size_t)2 * Bmax * dt * e);
    L.kcache = take((size_t)D.n_text_layer * Mmax * D.n_text_ctx * dt * e);
    L.vcache = take((size_t)D.n_text_layer * Mmax * D.n_text_ctx * dt * e);
    L.sk = take((size_t)Bmax * D.n_text_ctx * dt * e);
    L.sv = take((size_t)Bmax * D.n_text_ctx * dt * e);
    L.cap = take((size_t)Bmax * (n_align > 0 ? n_align : 1) * D.n_text_ctx * D.n_audio_ctx * 4);
    L.mean = take((size_t)Bmax * (n_align > 0 ? n_align : 1) * D.n_audio_ctx * 4);
    L.sd = take((size_t)Bmax * (n_align > 0 ? n_align : 1) * D.n_audio_ctx * 4);
    L.suppress = take((size_t)MAX_SUPPRESS * 4);
    {
        // f32 slabs of the one K-split projection (K = 4d): the decode step's rows, and every row of a multi-token pass
        // (Bmax windows x n_text_ctx tokens: 9.2 MB per window for large-v3)
        int64_t srows = Mmax > 160 ? Mmax : 160;
        if ((int64_t)Bmax * D.n_text_ctx > srows) srows = (int64_t)Bmax * D.n_text_ctx;
        const size_t mx = swx_dec_slab_floats((int)srows, dt, 4 * dt);
        L.slabs = take(mx * 4 + 256);
        L.slab_bytes = mx * 4;
    }
    // the alignment-head list lives with the workspace, not with the weights: views that share one weight arena
    // (swx_bind_weights on the same buffer) may be configured with different heads
    L.heads = take(sizeof(int32_t) * (size_t)D.n_text_layer * D.n_text_head);
    L.win_uid = take((size_t)Bmax * 4 + 256);
    L.total = cur;
}

// ---------------------------------------------------------------------------------------------- profiler
struct ProfRec { int cls; double work; hipEvent_t a, b; };
bool g_prof_enabled = false;
// A/B switches (SWX_FLAG_* in swx_kernels.h), set through swx_debug_flags() by tests and scripts; no environment variable
int g_debug_flags = SWX_DEFAULT_FLAGS;
std::vector<ProfRec> g_prof;
std::vector<hipEvent_t> g_pool;
size_t g_pool_next = 0;

hipEvent_t prof_event()
{
    if (g_pool_next == g_pool.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        g_pool.push_back(e);
    }
    return g_pool[g_pool_next++];
}

}  // namespace

bool swx_prof_on() { return g_prof_enabled; }
int swx_flags() { return g_debug_flags; }
void swx_prof_begin(int cls, double work, hipStream_t s)
{
    ProfRec r{cls, work, prof_event(), prof_event()};
    if (!r.a || !r.b) return;
    (void)hipEventRecord(r.a, s);
    g_prof.push_back(r);
}
void swx_prof_end(hipStream_t s)
{
    if (!g_prof.empty()) (void)hipEventRecord(g_prof.back().b, s);
}

// ================================================================================================== C ABI

extern "C" {

int swx_debug_flags(int flags)
{
    const int old = g_debug_flags;
    if (flags >= 0) g_debug_flags = flags;
    return old;
}

int swx_prof_enable(int on)
{
    g_prof_enabled = on != 0;
    if (on) { g_prof.clear(); g_pool_next = 0; }
    return 0;
}

// out[cls*3 + {0,1,2}] = {launches, total milliseconds, total work}; synchronises the device
int swx_prof_collect(double *out, int n_classes)
{
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return -100 - (int)e;
    for (int i = 0; i < n_classes * 3; ++i) out[i] = 0.0;
    for (auto &r : g_prof) {
        if (r.cls < 0 || r.cls >= n_classes) continue;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) continue;
        out[r.cls * 3 + 0] += 1.0;
        out[r.cls * 3 + 1] += (double)ms;
        out[r.cls * 3 + 2] += r.work;
    }
    g_prof.clear();
    g_pool_next = 0;
    (void)hipGetLastError();      // a failed elapsed-time query must not surface later as somebody else's launch error
    return PC_COUNT;
}

const char *swx_strerror(int code)
{
    switch (code) {
        case 0: return "ok";
        case -1: return "invalid argument";
        case -2: return "size out of range";
        case -3: return "unsupported filter width";
        case -4: return "gemm shape/alignment not supported";
        case -5: return "attention shape not supported";
        case -7: return "not implemented";
        case -8: return "workspace too small for this call";
        case -9: return "weights / workspace not bound";
        case -10: return "unknown tensor name";
        case -11: return "tensor size mismatch";
        case -20: return "not a FLAC stream";
        case -21: return "corrupt FLAC stream (bad header, reserved code or CRC mismatch)";
        case -22: return "unsupported FLAC stream";
        case -23: return "truncated FLAC stream";
        default: return code <= -100 ? "HIP runtime error (code = -100 - hipError_t)" : "unknown error";
    }
}

int swx_version(void) { return 1; }

int swx_model_create(const swx_dims *dims, int dtype, swx_model **out)
{
    if (!dims || !out || (dtype != SWX_F32 && dtype != SWX_F16)) return -1;
    if (dims->n_audio_state % 64 || dims->n_text_state % 64) return -1;
    if (dims->n_audio_state / dims->n_audio_head != 64 || dims->n_text_state / dims->n_text_head != 64) return -1;
    if (dims->n_text_ctx > 448 || dims->n_audio_ctx > 1500) return -2;
    swx_model *m = new swx_model();
    m->dims = *dims;
    m->dtype = dtype;
    m->esz = dtype == SWX_F16 ? 2 : 4;
    build_layout(m);
    default_alignment_heads(m);
    upload_heads(m);
    *out = m;
    return 0;
}

void swx_model_destroy(swx_model *m) { delete m; }

size_t swx_weights_bytes(const swx_model *m) { return m ? m->arena_bytes : 0; }

int swx_bind_weights(swx_model *m, void *d_arena, size_t bytes)
{
    if (m) m->drop_graphs();          // captured steps hold the old pointers
    if (!m || !d_arena || bytes < m->arena_bytes) return -1;
    m->arena = (unsigned char *)d_arena;
    hipError_t e = hipMemset(d_arena, 0, m->arena_bytes);
    if (e != hipSuccess) return -100 - (int)e;
    std::vector<double2> tw(SWX_N_FFT);
    for (int i = 0; i < SWX_N_FFT; ++i) {
        const double a = 2.0 * M_PI * (double)i / (double)SWX_N_FFT;
        tw[i].x = cos(a); tw[i].y = sin(a);
    }
    e = hipMemcpy(m->arena + m->o_twiddle, tw.data(), sizeof(double2) * SWX_N_FFT, hipMemcpyHostToDevice);
    if (e != hipSuccess) return -100 - (int)e;
    for (auto &kv : m->slots) kv.second.loaded = false;
    m->fold_state = std::make_shared<bool>(false);       // a new arena: a state of its own (views of the old one keep theirs)
    return upload_heads(m);
}

int swx_share_weights(swx_model *m, const swx_model *owner)
{
    // a second handle on an arena that is already populated: nothing is cleared or re-initialised (swx_bind_weights
    // zeroes the arena), the bookkeeping of which tensors are present is taken over from the owner
    if (!m || !owner || !owner->arena || m == owner) return -1;
    if (m->dtype != owner->dtype || m->arena_bytes != owner->arena_bytes || memcmp(&m->dims, &owner->dims, sizeof(swx_dims)) != 0)
        return -1;
    m->arena = owner->arena;
    m->fold_state = owner->fold_state;
    for (auto &kv : m->slots) {
        auto it = owner->slots.find(kv.first);
        kv.second.loaded = it != owner->slots.end() && it->second.loaded;
    }
    return upload_heads(m);
}

int swx_load_tensor(swx_model *m, const char *name, const float *d_src, int64_t numel, void *stream)
{
    if (!m || !m->arena) return -9;
    auto it = m->slots.find(name);
    if (it == m->slots.end()) return -10;
    Slot &sl = it->second;
    hipStream_t s = S(stream);
    if (sl.kind == SK_MAT) {
        if (numel != sl.rows * sl.cols) return -11;
        SWX_TRY(swx_copy_rows(m->dtype, d_src, sl.cols, m->arena + sl.off, sl.dst_ld, sl.rows, sl.cols, s));
    } else if (sl.kind == SK_CONV) {
        if (numel != sl.rows * sl.cols * 3) return -11;
        SWX_TRY(swx_copy_conv_w(m->dtype, d_src, (int)sl.rows, (int)sl.cols, (int)sl.dst_ld, m->arena + sl.off, s));
    } else {
        if (numel != sl.cols) return -11;
        hipError_t e = hipMemcpyAsync(m->arena + sl.off, d_src, (size_t)numel * 4, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return -100 - (int)e;
    }
    sl.loaded = true;
    *m->fold_state = false;   // the folded copies are stale until the next swx_weights_finalize (for every view of this arena)
    return 0;
}

int swx_weights_complete(const swx_model *m)
{
    if (!m) return 0;
    for (auto &kv : m->slots) if (!kv.second.loaded) return 0;
    return 1;
}

int swx_weights_mark_loaded(swx_model *m)
{
    // the arena was filled from outside (a peer's packed arena received over RCCL): every slot counts as present
    if (!m || !m->arena) return -9;
    for (auto &kv : m->slots) kv.second.loaded = true;
    return 0;
}

int swx_weights_finalize(swx_model *m, void *stream)
{
    if (!m || !m->arena) return -9;
    if (!m->has_fold) return 0;
    for (auto &kv : m->slots) if (!kv.second.loaded) return -9;
    hipStream_t s = S(stream);
    const int d = m->dims.n_text_state;
    for (auto &w : m->dec) {
        SWX_TRY(swx_fold_ln(m->arena + w.wqkv, m->A<float>(w.ln1_g), m->A<float>(w.ln1_b), m->A<float>(w.bqkv), m->arena + w.wqkv_f,
                            m->A<float>(w.qkv_c1), m->A<float>(w.qkv_c2), 3 * d, d, s));
        SWX_TRY(swx_fold_ln(m->arena + w.wcq, m->A<float>(w.lnx_g), m->A<float>(w.lnx_b), m->A<float>(w.bcq), m->arena + w.wcq_f,
                            m->A<float>(w.cq_c1), m->A<float>(w.cq_c2), d, d, s));
        SWX_TRY(swx_fold_ln(m->arena + w.w1, m->A<float>(w.ln2_g), m->A<float>(w.ln2_b), m->A<float>(w.b1), m->arena + w.w1_f,
                            m->A<float>(w.w1_c1), m->A<float>(w.w1_c2), 4 * d, d, s));
        SWX_TRY(swx_fold_ln(m->arena + w.wo, nullptr, nullptr, nullptr, m->arena + w.wo_p, nullptr, nullptr, d, d, s));
        SWX_TRY(swx_fold_ln(m->arena + w.wco, nullptr, nullptr, nullptr, m->arena + w.wco_p, nullptr, nullptr, d, d, s));
        SWX_TRY(swx_fold_ln(m->arena + w.w2, nullptr, nullptr, nullptr, m->arena + w.w2_p, nullptr, nullptr, d, 4 * d, s));
    }
    *m->fold_state = true;
    return 0;
}

int swx_missing_tensor(const swx_model *m, int index, char *buf, int buflen)
{
    int k = 0;
    for (auto &kv : m->slots)
        if (!kv.second.loaded) {
            if (k == index) { snprintf(buf, buflen, "%s", kv.first.c_str()); return 1; }
            ++k;
        }
    return 0;
}

int swx_set_alignment_heads(swx_model *m, const int32_t *pairs, int n_pairs)
{
    if (!m || (n_pairs > 0 && !pairs)) return -1;
    const swx_dims &D = m->dims;
    std::vector<std::vector<int>> by(D.n_text_layer);
    for (int i = 0; i < n_pairs; ++i) {
        const int l = pairs[2 * i], h = pairs[2 * i + 1];
        if (l < 0 || l >= D.n_text_layer || h < 0 || h >= D.n_text_head) return -1;
        by[l].push_back(h);
    }
    m->heads_by_layer = by;
    return upload_heads(m);
}

int swx_num_alignment_heads(const swx_model *m) { return m ? m->n_align : 0; }

size_t swx_workspace_bytes(const swx_model *m, int max_windows, int max_rows)
{
    if (!m || max_windows <= 0 || max_rows <= 0) return 0;
    swx_model::WsLayout L;
    ws_layout(m, max_windows, max_rows, m->n_align, L);
    return L.total;
}

int swx_bind_workspace(swx_model *m, void *d_ws, size_t bytes, int max_windows, int max_rows)
{
    if (m) m->drop_graphs();
    if (!m || !d_ws || max_windows <= 0 || max_rows <= 0) return -1;
    swx_model::WsLayout L;
    ws_layout(m, max_windows, max_rows, m->n_align, L);
    if (bytes < L.total) return -8;
    m->ws = (unsigned char *)d_ws;
    m->ws_bytes = bytes;
    m->max_windows = max_windows;
    m->max_rows = max_rows;
    m->ws_n_align = m->n_align;
    m->L = L;
    hipError_t e = hipMemset(m->ws + L.zeros_i32, 0, (size_t)(max_rows > max_windows ? max_rows : max_windows) * 4 + 256);
    if (e == hipSuccess) e = hipMemset(m->ws + L.ticket, 0, (size_t)SWX_DEC_TICKETS * 4);
    if (e != hipSuccess) return -100 - (int)e;
    if (!m->heads_flat.empty()) {
        e = hipMemcpy(m->ws + L.heads, m->heads_flat.data(), m->heads_flat.size() * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) return -100 - (int)e;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------------- mel
int swx_log_mel(swx_model *m, const float *d_pcm, int B, float *d_mel, int per_item_max, void *stream)
{
    if (!m || !m->arena || !m->ws) return -9;
    if (B > m->max_windows) return -8;
    return swx_mel_launch(d_pcm, B, m->A<float>(m->o_hann), m->A<double2>(m->o_twiddle), m->A<float>(m->o_filters),
                          m->dims.n_mels, d_mel, m->Wp<unsigned>(m->L.gmax), per_item_max, S(stream));
}

int swx_log_mel_ragged_grouped(swx_model *m, const float *d_pcm, const int32_t *n_valid, const int32_t *n_total, int B,
                               float *d_mel, int group, void *stream)
{
    if (!m || !m->arena || !m->ws) return -9;
    if (B <= 0) return 0;
    if (B > m->max_windows) return -8;
    if (group <= 0 || B % group) return -1;
    if (!n_valid || !n_total) return -2;
    std::vector<int32_t> lens((size_t)B * 2);
    for (int b = 0; b < B; ++b) {
        // torch.stft's reflect padding needs more than n_fft/2 samples; one extra block row of 8 frames is launched
        if (n_total[b] <= 200 || n_total[b] / 160 > 3008 || n_valid[b] < 0 || n_valid[b] > n_total[b] ||
            n_valid[b] > 480000)
            return -2;
        lens[2 * b] = n_valid[b];
        lens[2 * b + 1] = n_total[b];
    }
    hipStream_t s = S(stream);
    int32_t *d_lens = m->Wp<int32_t>(m->L.h1);          // encoder scratch, idle while the spectrogram is computed
    hipError_t e = hipMemcpyAsync(d_lens, lens.data(), lens.size() * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);   // lens is a stack-lifetime staging buffer
    if (e != hipSuccess) return -100 - (int)e;
    return swx_mel_ragged_launch(d_pcm, d_lens, B, m->A<float>(m->o_hann), m->A<double2>(m->o_twiddle),
                                 m->A<float>(m->o_filters), m->dims.n_mels, d_mel, m->Wp<unsigned>(m->L.gmax), group, s);
}

int swx_log_mel_ragged(swx_model *m, const float *d_pcm, const int32_t *n_valid, const int32_t *n_total, int B,
                       float *d_mel, int per_item_max, void *stream)
{
    return swx_log_mel_ragged_grouped(m, d_pcm, n_valid, n_total, B, d_mel, per_item_max ? 1 : B, stream);
}

// ----------------------------------------------------------------------------------------------------- encoder
int swx_encode(swx_model *m, const float *d_mel, int B, void *d_xa, void *stream)
{
    if (!m || !m->arena || !m->ws) return -9;
    if (B <= 0) return 0;
    if (B > m->max_windows) return -8;
    const swx_dims &D = m->dims;
    const int d = D.n_audio_state, H = D.n_audio_head, S_ = D.n_audio_ctx;
    const size_t e = m->esz;
    hipStream_t s = S(stream);
    unsigned char *melT = m->ws + m->L.melT, *h1 = m->ws + m->L.h1;
    unsigned char *x = m->ws + m->L.x, *h = m->ws + m->L.h, *qkv = m->ws + m->L.qkv, *att = m->ws + m->L.att, *u = m->ws + m->L.u;
    const int rows = B * S_;
    if (D.n_audio_ctx != 1500) return -2;

    SWX_TRY(swx_mel_transpose(m->dtype, d_mel, B, D.n_mels, m->Cp, melT, s));
    // conv1 (k=3, pad 1) as a GEMM over overlapping rows of the channel-last mel: A row t = melT[t .. t+2][:]
    SWX_TRY(swx_fill_zero(h1, (size_t)B * 3002 * d * e, s));
    for (int b = 0; b < B; ++b) {
        const unsigned char *a = melT + (size_t)b * 3002 * m->Cp * e;
        unsigned char *c = h1 + ((size_t)b * 3002 + 1) * d * e;
        SWX_TRY(swx_gemm(m->dtype, swx_gemm_args(a, m->Cp, m->arena + m->o_conv1_w, 3 * m->Cp, m->A<float>(m->o_conv1_b), c, d,
                                             3000, d, 3 * m->Cp, EPI_BIAS | EPI_GELU), 0, s));
    }
    // conv2 (k=3, stride 2, pad 1): A row t' = h1[2t' .. 2t'+2][:] (padded row index), then + positional embedding
    for (int b = 0; b < B; ++b) {
        const unsigned char *a = h1 + (size_t)b * 3002 * d * e;
        GemmArgs g = swx_gemm_args(a, 2 * d, m->arena + m->o_conv2_w, 3 * d, m->A<float>(m->o_conv2_b), x + (size_t)b * S_ * d * e, d,
                               S_, d, 3 * d, EPI_BIAS | EPI_GELU | EPI_RESF32MOD);
        g.Rf = m->A<float>(m->o_enc_pos); g.res_mod = S_;
        SWX_TRY(swx_gemm(m->dtype, g, 0, s));
    }
    for (int l = 0; l < D.n_audio_layer; ++l) {
        const LayerW &w = m->enc[l];
        SWX_TRY(swx_layernorm(m->dtype, x, d, m->A<float>(w.ln1_g), m->A<float>(w.ln1_b), h, d, rows, d, s));
        // f16 at few windows (wherever the launch does not go to the 256 x 256 kernel, whose epilogue is plain): V leaves the
        // projection's epilogue transposed per head (EPI_QKV_VT, round 6) instead of by a launch of its own -- 5 us x 32 layers per
        // window pass of align(); the `u` buffer (MLP hidden, 4d wide) is free until the MLP of this layer
        const bool fuse_vt = m->dtype == SWX_F16 && d % 128 == 0 && S_ % 4 == 0 && !(g_debug_flags & SWX_FLAG_QKV_SEPARATE_VT) &&
                             swx_gemm_plan_f16(rows, 3 * d, d, EPI_BIAS, 3 * d, 1, true, 0, g_debug_flags) != SWX_GEMM_BIG;
        {
            GemmArgs gq = swx_gemm_args(h, d, m->arena + w.wqkv, d, m->A<float>(w.bqkv), qkv, 3 * d, rows, 3 * d, d, EPI_BIAS | (fuse_vt ? EPI_QKV_VT : 0));
            if (fuse_vt) { gq.C2 = u; gq.vt_s = S_; gq.vt_kp = SWX_VT_KP; gq.vt_bs = (int64_t)H * 64 * SWX_VT_KP; gq.vt_zero_pad = 1; }
            SWX_TRY(swx_gemm(m->dtype, gq, 0, s));
        }
        AttnArgs a{};
        a.q = qkv; a.ldq = 3 * d; a.k = qkv + (size_t)d * e; a.v = qkv + (size_t)2 * d * e; a.ldkv = 3 * d; a.o = att; a.ldo = d;
        a.k_bs = (int64_t)S_ * 3 * d; a.v_bs = a.k_bs; a.vt_kp = 0;
        a.B = B; a.H = H; a.nq = S_; a.nk = S_; a.q_rows_per_batch = S_;
        if (m->dtype == SWX_F16) {
            // V of this layer transposed per head (one streaming pass, ~35 us for 20 windows): the flash kernel then stages both
            // operands with 16-byte vector stores; the `u` buffer (MLP hidden, 4d wide) is free until the MLP of this layer
            if (!fuse_vt) SWX_TRY(swx_transpose_v(a.v, 3 * d, a.v_bs, S_, u, SWX_VT_KP, (int64_t)H * 64 * SWX_VT_KP, B, H, s));
            a.v = u; a.vt_kp = SWX_VT_KP; a.v_bs = (int64_t)H * 64 * SWX_VT_KP;
        }
        SWX_TRY(swx_attention(m->dtype, a, 0, s));
        SWX_TRY(swx_gemm_residual(m, att, d, w.wo, w.bo, x, d, rows, d, d, s));
        SWX_TRY(swx_layernorm(m->dtype, x, d, m->A<float>(w.ln2_g), m->A<float>(w.ln2_b), h, d, rows, d, s));
        SWX_TRY(swx_gemm(m->dtype, swx_gemm_args(h, d, m->arena + w.w1, d, m->A<float>(w.b1), u, 4 * d, rows, 4 * d, d, EPI_BIAS | EPI_GELU), 0, s));
        SWX_TRY(swx_gemm_residual(m, u, 4 * d, w.w2, w.b2, x, d, rows, d, 4 * d, s));
    }
    SWX_TRY(swx_layernorm(m->dtype, x, d, m->A<float>(m->o_lnpost_g), m->A<float>(m->o_lnpost_b), d_xa, d, rows, d, s));
    return 0;
}

size_t swx_cross_kv_bytes(const swx_model *m, int B)
{
    if (!m) return 0;
    return (size_t)m->dims.n_text_layer * B * (size_t)xkv_chunk_elems(m) * m->esz;
}

int swx_cross_kv(swx_model *m, const void *d_xa, int B, void *d_xkv, void *stream)
{
    if (!m || !m->arena) return -9;
    const swx_dims &D = m->dims;
    const int d = D.n_text_state, S_ = D.n_audio_ctx;
    const size_t e = m->esz;
    if (D.n_audio_state != d) return -1;
    const int64_t chunk = xkv_chunk_elems(m);
    hipStream_t s = S(stream);
    // the key padding of V^T (columns S_..KP of each of the d rows of every layer's / window's V^T block) must be finite: it is
    // multiplied by exact-zero probabilities.  Everything else in the buffer is written below (K rows, V^T columns, packed copy).
    SWX_TRY(swx_pad_zero((unsigned char *)d_xkv + (size_t)S_ * d * e, (int64_t)SWX_VT_KP * e, chunk * (int64_t)e, (int)(S_ * e),
                         (int)((SWX_VT_KP - S_) * e), d, D.n_text_layer * B, s));
    for (int l = 0; l < D.n_text_layer; ++l) {
        const LayerW &w = m->dec[l];
        unsigned char *base = (unsigned char *)d_xkv + (size_t)l * B * chunk * e;
        const bool one_launch = m->dtype == SWX_F16 && d % 128 == 0 && (int64_t)B * S_ > 128 && !(g_debug_flags & SWX_FLAG_XKV_TWO_LAUNCHES);
        bool packed_by_epilogue = false;
        if (one_launch) {
            // round 6: K and V of the layer from ONE launch over the fused weight rows [2d][d] (EPI_KV: a tile left of column d stores
            // K rows per window, a tile right of it V transposed per head) -- at one window 240 tiles of 128 x 128 on the ring kernel
            // instead of two launches of 240 tiles of 128 x 64; per element the same MFMA sequence, so bit-identical
            GemmArgs gkv = swx_gemm_args(d_xa, d, m->arena + w.wckv, d, m->A<float>(w.bckv), base, d, B * S_, 2 * d, d, EPI_BIAS | EPI_KV);
            gkv.vt_s = S_; gkv.vt_kp = SWX_VT_KP; gkv.vt_bs = chunk; gkv.C2 = base + (size_t)S_ * d * e;
            if (!(g_debug_flags & SWX_FLAG_XKV_PACK_SEPARATE)) {
                // ... and the fragment-ordered copy from the same epilogue (round 6: swx_xkv_pack read and wrote the layer's K / V^T once more)
                gkv.P = base + (size_t)xkv_plain_elems(D) * e; gkv.p_bs = chunk; gkv.p_nkpad = ((S_ + 31) / 32) * 32; gkv.p_vcol0 = d;
                packed_by_epilogue = true;
            }
            SWX_TRY(swx_gemm(m->dtype, gkv, 0, s));
        } else {
        // K (no bias upstream; the fused bias slot is zero): one GEMM over all windows, rows scattered per window chunk
        GemmArgs gk = swx_gemm_args(d_xa, d, m->arena + w.wckv, d, m->A<float>(w.bckv), base, d, B * S_, d, d, EPI_BIAS | EPI_CBATCH);
        gk.vt_s = S_; gk.vt_kp = 0; gk.vt_bs = chunk;
        SWX_TRY(swx_gemm(m->dtype, gk, 0, s));
        // V, stored transposed per head behind each window's K
        GemmArgs gv = swx_gemm_args(d_xa, d, m->arena + w.wckv + (size_t)d * d * e, d, m->A<float>(w.bckv) + d,
                                base + (size_t)S_ * d * e, d, B * S_, d, d, EPI_BIAS | EPI_STORE_VT);
        gv.vt_s = S_; gv.vt_kp = SWX_VT_KP; gv.vt_bs = chunk;
        SWX_TRY(swx_gemm(m->dtype, gv, 0, s));
        }
        if (m->dtype == SWX_F16 && !packed_by_epilogue)      // the decode-step cross-attention streams the fragment-ordered copy
            SWX_TRY(swx_xkv_pack(base, base + (size_t)S_ * d * e, base + (size_t)xkv_plain_elems(D) * e, B, D.n_text_head, S_, d,
                                 SWX_VT_KP, chunk, s));
    }
    return 0;
}

// d_out[e] = sum_j coef[j] * d_xs[j][e], n_in <= 8 (extra_models: the pooled matrix from each model's own head mean)
int swx_weighted_sum(const float *const *h_xs, const float *h_coef, int n_in, float *d_out, int64_t n, void *stream)
{
    if (!h_xs || !h_coef || !d_out) return -1;
    return swx_weighted_sum_launch(h_xs, h_coef, n_in, d_out, n, S(stream));
}

// how the decode loops of this handle ran so far: out[0] = step graphs captured, out[1] = two-step graph replays,
// out[2] = steps launched eagerly, out[3] = 1 when capture / replay failed once and the handle fell back to eager launches
int swx_graph_stats(const swx_model *m, int64_t *out)
{
    if (!m || !out) return -1;
    out[0] = m->n_captures; out[1] = m->n_replays; out[2] = m->n_eager_units; out[3] = (m->graphs_off || m->graph_failures > 0) ? 1 : 0;
    return 0;
}

}  // extern "C"
