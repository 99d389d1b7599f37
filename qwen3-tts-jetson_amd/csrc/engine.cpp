// engine.cpp — see engine.h.  (Continuous batching, Engine::generate_queue, is engine_queue.cpp.)
#include "engine_internal.h"
#include "persist.h"

#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sys/stat.h>
#include <algorithm>
#include <condition_variable>
#include <mutex>

#include "devlock.h"
#include <chrono>
#include "speaker.h"
#include "vocoder.h"

namespace q3t {

Engine::Engine() = default;

namespace {
WPLock g_device_rw[64];
thread_local int t_device_depth[64];
}  // namespace

// devlock.h: exclusive for single-slot (persistent-kernel) runs, shared for everything else
DeviceLock::DeviceLock(bool exclusive, int device) : dev_(device & 63) {
    if (t_device_depth[dev_]++ > 0) return;
    mode_ = exclusive ? 2 : 1;
    if (exclusive) g_device_rw[dev_].lock();
    else g_device_rw[dev_].lock_shared();
}
DeviceLock::~DeviceLock() {
    --t_device_depth[dev_];
    if (mode_ == 2) g_device_rw[dev_].unlock();
    else if (mode_ == 1) g_device_rw[dev_].unlock_shared();
}

namespace {
int env_int(const char *name, int dflt) {
    const char *e = std::getenv(name);
    return e ? std::atoi(e) : dflt;
}
bool env_flag(const char *name, bool dflt) { return env_int(name, dflt) != 0; }
}  // namespace

Options Options::from_env() {
    Options o;
    o.persist = env_flag("Q3T_PERSIST", true);
    o.persist_cp = env_flag("Q3T_PERSIST_CP", true);
    o.cp_fused_attn = env_flag("Q3T_CP_FUSED_ATTN", true);
    o.cp_qkv_table = env_flag("Q3T_CP_QKV_TABLE", true);
    o.cp_roles = env_flag("Q3T_CP_ROLES", true);
    o.mm_cp_table = env_flag("Q3T_MM_CP_TABLE", true);
    o.fold_advance = env_flag("Q3T_FOLD_ADVANCE", true);
    o.tk_roles = env_flag("Q3T_TK_ROLES", true);
    o.cpb = env_flag("Q3T_PERSIST_CPB", true);
    o.tkb = env_flag("Q3T_PERSIST_TKB", true);
    o.fused_select = env_flag("Q3T_FUSED_SELECT", true);
    o.defer_cp_select = env_flag("Q3T_CP_DEFER_SELECT", true);
    o.attn_split = env_flag("Q3T_ATTN_SPLIT", false);
    // models with code_pred.mtp_proj (1.7B) on the batched matrix-core stack; 0: every projection of such a model on the
    // vector kernels with a 1-slot K split at any batch size, as before the stack covered them
    o.mm17 = env_flag("Q3T_MM17", true);
    // weight prefetch of the batched talker stack: 0 off (default), 1 the norms before QKV and gate/up, 2 also the gate/up
    // GEMM for the down projection (its 64-token tiles leave a quarter of the CUs free).  Off since round 5: level 2 saved
    // 0.3 % of the 64-slot step (1.5960 -> 1.5912 ms, two A/B pairs) for 755 MB more fabric reads per step (FETCH 3,111 ->
    // 3,866 MB: every prefetched line is read twice, once into the Infinity Cache and once by the GEMM)
    o.mm_prefetch = env_int("Q3T_MM_PREFETCH", 0);
    // gate/up on 64-token tiles: 192 workgroups of one per CU instead of 384 (two on half the CUs, which set the tail);
    // the other projections keep 32-token tiles.  64-slot talker step 1.574 -> 1.549 ms (two A/B pairs,
    // tools/dev/exp_gutt.sh); the tile never changes a row's arithmetic.  Q3T_MM_GU_TT=1 restores 32-token tiles.
    o.mm_gu_tt = env_int("Q3T_MM_GU_TT", 2);
    if (const char *e = std::getenv("Q3T_PERSIST_FAULT_AT")) o.persist_fault_at = (unsigned)std::max(0, std::atoi(e));
#ifdef Q3T_DEV
    if (const char *e = std::getenv("Q3T_POLL_EVERY")) o.poll_every = std::max(1, std::atoi(e));
#endif
    return o;
}

Engine::~Engine() {
    if (device_ >= 0) hipSetDevice(device_);
    for (auto &kv : g_talker_) hipGraphExecDestroy(kv.second);
    for (auto &kv : g_frame_) hipGraphExecDestroy(kv.second);
    for (auto &kv : g_prefill_) hipGraphExecDestroy(kv.second);
    for (auto &kv : g_prefill_rag_) hipGraphExecDestroy(kv.second);
    for (auto &kv : g_cp_) hipGraphExecDestroy(kv.second);
    voc_.reset();
    for (void *p : allocs_) hipFree(p);
    if (qout_) hipFree(qout_);
    if (qstage_) hipFree(qstage_);
    if (pin_) hipHostFree(pin_);
    for (PinnedChunk &c : chunk_pool_) { hipHostFree(c.codes); hipEventDestroy(c.ev); }
    for (int b = 0; b < FeedScratch::NBUF; ++b) {
        if (feed_.pin[b]) hipHostFree(feed_.pin[b]);
        if (feed_.e0[b]) hipEventDestroy(feed_.e0[b]);
        if (feed_.e1[b]) hipEventDestroy(feed_.e1[b]);
    }
    if (stream_) hipStreamDestroy(stream_);
    if (astream_) hipStreamDestroy(astream_);
}


// the pinned / device scratch of generate() and generate_queue(), kept across calls: a per-call hipFree or
// hipHostFree would synchronise the whole device (every other context on it included)
bool Engine::ensure_pinned(size_t bytes) {
    if (bytes <= pin_cap_) return true;
    if (pin_) hipHostFree(pin_);
    pin_ = nullptr;
    pin_cap_ = 0;
    if (hipHostMalloc(&pin_, bytes, hipHostMallocDefault) != hipSuccess) { pin_ = nullptr; set_error("hipHostMalloc failed"); return false; }
    pin_cap_ = bytes;
    return true;
}
bool Engine::ensure_device(void *&p, size_t &cap, size_t bytes) {
    if (bytes <= cap) return true;
    if (p) hipFree(p);
    p = nullptr;
    cap = 0;
    if (hipMalloc(&p, bytes) != hipSuccess) { p = nullptr; set_error("device allocation failed"); return false; }
    cap = bytes;
    return true;
}
bool Engine::pinned_chunk(size_t idx, size_t bytes, PinnedChunk **out) {
    while (chunk_pool_.size() <= idx) chunk_pool_.push_back(PinnedChunk{});
    PinnedChunk &pc = chunk_pool_[idx];
    if (pc.cap < bytes) {
        if (pc.codes) hipHostFree(pc.codes);
        pc.codes = nullptr;
        pc.cap = 0;
        Q3T_HIP(hipHostMalloc(&pc.codes, bytes, hipHostMallocDefault));
        pc.cap = bytes;
    }
    if (!pc.ev) Q3T_HIP(hipEventCreateWithFlags(&pc.ev, hipEventDisableTiming));
    *out = &pc;
    return true;
}

namespace {
bool check_shape(const GgufTensor *t, const char *name, int64_t cols, int64_t rows, int type) {
    if (!t) { set_error(std::string("missing tensor ") + name); return false; }
    const bool lead_ok = t->ne[0] == cols || (t->n_dims == 3 && t->ne[0] == 1 && t->ne[1] == cols);
    if (t->type != type || !lead_ok || t->nelements() != cols * rows) {
        set_error(std::string("tensor ") + name + ": unexpected shape/type");
        return false;
    }
    return true;
}
}  // namespace

// parse_config key aliases / defaults: src/tts_transformer.cpp:288-442 (GGUF header keys only: every rank, and the
// host-only layout plan, compute the same config)
bool Engine::parse_config(const Gguf &g) {
    c_.text_vocab = (int)g.get_int({"qwen3-tts.text.vocab_size", "qwen3-tts.text_vocab_size"}, 151936);
    c_.text_dim = (int)g.get_int({"qwen3-tts.text.embedding_dim", "qwen3-tts.text_hidden_size"}, 2048);
    c_.hidden = (int)g.get_int({"qwen3-tts.talker.embedding_length", "qwen3-tts.embedding_length"}, 1024);
    c_.n_layers = (int)g.get_int({"qwen3-tts.talker.block_count", "qwen3-tts.block_count"}, 28);
    c_.n_heads = (int)g.get_int({"qwen3-tts.talker.attention.head_count", "qwen3-tts.attention.head_count"}, 16);
    c_.n_kv = (int)g.get_int({"qwen3-tts.talker.attention.head_count_kv", "qwen3-tts.attention.head_count_kv"}, 8);
    c_.inter = (int)g.get_int({"qwen3-tts.talker.feed_forward_length", "qwen3-tts.feed_forward_length"}, 3072);
    c_.head_dim = (int)g.get_int({"qwen3-tts.talker.attention.key_length", "qwen3-tts.attention.key_length"}, 128);
    c_.eps = g.get_f32({"qwen3-tts.talker.attention.layer_norm_rms_epsilon", "qwen3-tts.attention.layer_norm_rms_epsilon"}, 1e-6f);
    c_.rope_theta = g.get_f32({"qwen3-tts.talker.rope.freq_base", "qwen3-tts.rope.freq_base"}, 1000000.0f);
    c_.codec_vocab = (int)g.get_int({"qwen3-tts.talker.codec_vocab_size", "qwen3-tts.vocab_size"}, 3072);
    c_.n_codebooks = (int)g.get_int({"qwen3-tts.talker.num_codebooks", "qwen3-tts.num_code_groups"}, 16);
    c_.cp_layers = (int)g.get_int({"qwen3-tts.code_pred.layer_count", "qwen3-tts.code_predictor.layer_count"}, 5);
    c_.cp_vocab = (int)g.get_int({"qwen3-tts.code_pred.vocab_size", "qwen3-tts.code_predictor.vocab_size"}, 2048);
    c_.codec_pad = (int)g.get_int({"qwen3-tts.codec.pad_id"}, 2148);
    c_.codec_bos = (int)g.get_int({"qwen3-tts.codec.bos_id"}, 2149);
    c_.codec_eos = (int)g.get_int({"qwen3-tts.codec.eos_id", "qwen3-tts.codec.eos_token_id"}, 2150);
    c_.tts_bos = (int)g.get_int({"qwen3-tts.tts_bos_token_id", "qwen3-tts.tts.bos_token_id", "qwen3-tts.tts.bos_id"}, 151672);
    c_.tts_eos = (int)g.get_int({"qwen3-tts.tts_eos_token_id", "qwen3-tts.tts.eos_token_id", "qwen3-tts.tts.eos_id"}, 151673);
    c_.tts_pad = (int)g.get_int({"qwen3-tts.tts_pad_token_id", "qwen3-tts.tts.pad_token_id", "qwen3-tts.tts.pad_id"}, 151671);
    c_.think = (int)g.get_int({"qwen3-tts.codec.think_id", "qwen3-tts.codec_think_id"}, 2154);
    c_.nothink = (int)g.get_int({"qwen3-tts.codec.nothink_id", "qwen3-tts.codec_nothink_id"}, 2155);
    c_.think_bos = (int)g.get_int({"qwen3-tts.codec.think_bos_id", "qwen3-tts.codec_think_bos_id"}, 2156);
    c_.think_eos = (int)g.get_int({"qwen3-tts.codec.think_eos_id", "qwen3-tts.codec_think_eos_id"}, 2157);
    // code predictor architecture (falls back to the talker's values: 0.6B), tts_transformer.cpp:370-389
    c_.cp_hidden = (int)g.get_int({"qwen3-tts.code_predictor.embedding_length"}, c_.hidden);
    c_.cp_inter = (int)g.get_int({"qwen3-tts.code_predictor.feed_forward_length"}, c_.inter);
    c_.cp_heads = (int)g.get_int({"qwen3-tts.code_predictor.attention.head_count"}, c_.n_heads);
    c_.cp_kv = (int)g.get_int({"qwen3-tts.code_predictor.attention.head_count_kv"}, c_.n_kv);
    const int cp_head_dim = (int)g.get_int({"qwen3-tts.code_predictor.attention.key_length"}, c_.head_dim);
    c_.has_mtp = g.find("code_pred.mtp_proj.weight") != nullptr;
    if (c_.cp_hidden != c_.hidden && !c_.has_mtp) {
        set_error("code predictor hidden != talker hidden without code_pred.mtp_proj");
        return false;
    }
    if (cp_head_dim != c_.head_dim) { set_error("code predictor head_dim must equal the talker's (shared RoPE table)"); return false; }
    cpc_ = c_;
    cpc_.hidden = c_.cp_hidden; cpc_.inter = c_.cp_inter; cpc_.n_heads = c_.cp_heads; cpc_.n_kv = c_.cp_kv;
    // the batched matrix-core stack (hoisted norms, k_resid_norm): widths <= 1024 without code_pred.mtp_proj (0.6B); with
    // it (1.7B) a talker up to 2,048 wide over a code predictor up to 1,024 wide whose every projection is a shape of
    // the MFMA GEMM (Q3T_MM17=0: off).  Other models run every projection on the vector kernels with a 1-slot K split
    // at any batch size.
    auto mm_stack_shapes = [](const Config &k, int head_vocab) {
        auto kdim = [](int K) { return K == 256 || K == 512 || K == 1024 || K == 2048 || K == 3072; };
        const int A = k.n_heads * k.head_dim, QKV = (k.n_heads + 2 * k.n_kv) * k.head_dim;
        // (K of QKV / gate-up / head, of the O projection, of the down projection -- slabs only at 6,144; N in 32-row tiles)
        return kdim(k.hidden) && kdim(A) && (kdim(k.inter) || k.inter == 6144) && QKV % 32 == 0 && head_vocab % 32 == 0;
    };
    mm_ok_ = c_.has_mtp ? opt_.mm17 && c_.hidden <= 2048 && c_.cp_hidden <= 1024 && mm_stack_shapes(c_, c_.codec_vocab) &&
                              mm_stack_shapes(cpc_, c_.cp_vocab)
                        : c_.hidden <= 1024 && c_.cp_hidden <= 1024;
    fam1_ = mm_ok_ ? 0 : 1;
    if (c_.n_codebooks != 16) { set_error("n_codebooks must be 16"); return false; }
    // the fused code-predictor attention prologue is specialised to the 0.6B head layout (16 q / 8 kv heads x 128)
    cp_fused_attn_ = cp_fused_attn_ && c_.cp_heads == 16 && c_.cp_kv == 8 && c_.head_dim == 128 && c_.cp_hidden == 1024;
    return true;
}

bool Engine::load(const std::string &tts_gguf, const std::string &tok_gguf, int device, int max_slots, int max_ctx,
                  bool recv_weights) {
    DeviceLock lk(false, device);   // allocation zeroing / weight upload run kernels and copies on this device
    device_ = device;
    tts_path_ = tts_gguf;
    tok_path_ = tok_gguf;
    wa_.recv = recv_weights;
    opt_ = Options::from_env();
    cp_fused_attn_ = opt_.cp_fused_attn;
    defer_cp_select_ = opt_.defer_cp_select;
    fused_select_ = opt_.fused_select;
    persist_ = opt_.persist;
    poll_every_ = opt_.poll_every;
    max_slots_ = std::max(1, max_slots);
    max_ctx_ = std::max(32, max_ctx);
    if (max_ctx_ > ATTN_CHUNK * ATTN_MAX_SPLITS) { set_error("max_ctx exceeds " + std::to_string(ATTN_CHUNK * ATTN_MAX_SPLITS)); return false; }
    Q3T_HIP(hipSetDevice(device));
    Q3T_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    if (tts_gguf.empty()) {
        // vocoder-only context (AudioTokenizerDecoder / TRTVocoderDecoder load without a talker model)
        if (tok_gguf.empty()) { set_error("no model file given"); return false; }
        talker_ = false;
        voc_.reset(new Vocoder());
        if (!voc_->load(tok_gguf, stream_, recv_weights)) return false;
        Q3T_HIP(hipStreamSynchronize(stream_));
        return true;
    }
    Gguf g;
    if (!g.open(tts_gguf)) { set_error(g.error()); return false; }
    if (!parse_config(g)) return false;
    if (!upload_weights(g)) return false;
    if (!alloc_state()) return false;
#ifdef Q3T_DEV
    if (const char *e = std::getenv("Q3T_TALKER_LAYERS")) {   // truncated talker stack (development builds only)
        const int n = std::atoi(e);
        if (n > 0 && n < c_.n_layers) { c_.n_layers = n; L_.resize(n); }
    }
#endif
    int n_cu = 0;
    Q3T_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device_));
    if (!setup_persist(n_cu)) return false;
    if (!setup_cpb(n_cu)) return false;
    if (!setup_tkb(n_cu)) return false;
#ifdef Q3T_DEV
    // development timeline of whichever persistent launch runs (read back through debug_read 5)
    if ((persist_ || persist_cp_ || cpb_ || tkb_) && std::getenv("Q3T_PERSIST_PROF")) pprof_ = dalloc<uint64_t>((size_t)PROF_WG * PROF_PH * 4);
#endif
    if (!tok_gguf.empty()) {
        voc_.reset(new Vocoder());
        if (!voc_->load(tok_gguf, stream_, recv_weights)) return false;
    }
    Q3T_HIP(hipStreamSynchronize(stream_));
    return true;
}

bool Engine::load_speaker_only(const std::string &tts_gguf, int device) {
    DeviceLock lk(false, device);
    device_ = device;
    tts_path_ = tts_gguf;
    talker_ = false;
    Q3T_HIP(hipSetDevice(device));
    Q3T_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    Gguf g;
    if (!g.open(tts_gguf)) { set_error(g.error()); return false; }
    size_t total = 0;
    for (const GgufTensor &t : g.tensors())
        if (t.name.rfind("spk_enc.", 0) == 0) total += (t.nbytes() + 255) & ~(size_t)255;
    if (total == 0) { set_error("No speaker encoder tensors found in model"); return false; }
    if (!wa_.reserve(total + ((size_t)1 << 20))) return false;
    spk_.reset(new SpeakerEncoder());
    if (!spk_->load(g, wa_, stream_)) return false;
    Q3T_HIP(hipStreamSynchronize(stream_));
    return true;
}

std::vector<WeightArena *> Engine::weight_arenas() {
    std::vector<WeightArena *> v{&wa_};
    if (voc_ && voc_->loaded()) v.push_back(&voc_->weights());
    return v;
}

bool Engine::upload_weights(const Gguf &g) { return layout_weights(g) && upload_weights_rest(); }

// every weight tensor into the arena, in a fixed order that depends on the GGUF shapes alone
bool Engine::layout_weights(const Gguf &g) {
    const int H = c_.hidden, D = c_.head_dim;
    // every weight goes into the arena (one blob: the unit of the RCCL broadcast); receiving ranks touch only the
    // GGUF headers, never the tensor bytes
    size_t total = 0;
    for (const GgufTensor &t : g.tensors()) total += (t.nbytes() + 255) & ~(size_t)255;
    if (!wa_.reserve(total + ((size_t)1 << 20))) return false;
    const bool recv = wa_.recv;
    auto up16 = [&](const char *name, int64_t cols, int64_t rows) -> uint16_t * {
        const GgufTensor *t = g.find(name);
        if (!check_shape(t, name, cols, rows, GGML_TYPE_F16)) return nullptr;
        uint16_t *d = wa_.alloc<uint16_t>((size_t)cols * rows);
        if (!d || !wa_.put(d, t->data, t->nbytes())) return nullptr;
        return d;
    };
    auto up32 = [&](const char *name, int64_t n) -> float * {
        const GgufTensor *t = g.find(name);
        if (!t || t->type != GGML_TYPE_F32 || t->nelements() != n) { set_error(std::string("bad f32 tensor ") + name); return nullptr; }
        float *d = wa_.alloc<float>((size_t)n);
        if (!d || !wa_.put(d, t->data, t->nbytes())) return nullptr;
        return d;
    };
    auto rows16 = [&](const std::string &name, int64_t cols, int64_t rows, std::vector<uint16_t> &dst, size_t at) -> bool {
        const GgufTensor *t = g.find(name);
        if (!check_shape(t, name.c_str(), cols, rows, GGML_TYPE_F16)) return false;
        if (!recv) std::memcpy(dst.data() + at, t->data, t->nbytes());
        return true;
    };
    auto layer = [&](const char *pfx, int i, DevLayer &l, const Config &lc) -> bool {
        const int H = lc.hidden, Dq = lc.n_heads * D, Dkv = lc.n_kv * D, I = lc.inter;
        if (I % 16 != 0 || H % 8 != 0) { set_error("unsupported hidden/intermediate size"); return false; }
        char b[160];
        auto nm = [&](const char *s) { snprintf(b, sizeof b, "%s.blk.%d.%s", pfx, i, s); return std::string(b); };
        // fused [Wq; Wk; Wv] rows
        const size_t n_qkv = (size_t)(Dq + 2 * Dkv) * H;
        std::vector<uint16_t> qkv(recv ? 0 : n_qkv);
        if (!rows16(nm("attn_q.weight"), H, Dq, qkv, 0) || !rows16(nm("attn_k.weight"), H, Dkv, qkv, (size_t)Dq * H) ||
            !rows16(nm("attn_v.weight"), H, Dkv, qkv, (size_t)(Dq + Dkv) * H))
            return false;
        if (!(l.qkv = wa_.alloc<uint16_t>(n_qkv)) || !wa_.put(l.qkv, qkv.data(), n_qkv * 2)) return false;
        // gate/up interleaved in 16-row blocks (k_gemv ACT_SWIGLU layout)
        const size_t n_gu = (size_t)2 * I * H;
        std::vector<uint16_t> gate(recv ? 0 : (size_t)I * H), up(recv ? 0 : (size_t)I * H), gu(recv ? 0 : n_gu);
        if (!rows16(nm("ffn_gate.weight"), H, I, gate, 0) || !rows16(nm("ffn_up.weight"), H, I, up, 0)) return false;
        if (!recv)
            for (int blk = 0; blk < I / 16; ++blk) {
                std::memcpy(gu.data() + (size_t)(blk * 32) * H, gate.data() + (size_t)(blk * 16) * H, (size_t)16 * H * 2);
                std::memcpy(gu.data() + (size_t)(blk * 32 + 16) * H, up.data() + (size_t)(blk * 16) * H, (size_t)16 * H * 2);
            }
        if (!(l.gu = wa_.alloc<uint16_t>(n_gu)) || !wa_.put(l.gu, gu.data(), n_gu * 2)) return false;
        if (!(l.o = up16(nm("attn_output.weight").c_str(), Dq, H))) return false;
        if (!(l.down = up16(nm("ffn_down.weight").c_str(), I, H))) return false;
        if (!(l.attn_norm = up32(nm("attn_norm.weight").c_str(), H))) return false;
        if (!(l.ffn_norm = up32(nm("ffn_norm.weight").c_str(), H))) return false;
        if (!(l.qn = up32(nm("attn_q_norm.weight").c_str(), D))) return false;
        if (!(l.kn = up32(nm("attn_k_norm.weight").c_str(), D))) return false;
        return true;
    };
    L_.resize(c_.n_layers);
    CP_.resize(c_.cp_layers);
    for (int i = 0; i < c_.n_layers; ++i) if (!layer("talker", i, L_[i], c_)) return false;
    for (int i = 0; i < c_.cp_layers; ++i) if (!layer("code_pred", i, CP_[i], cpc_)) return false;
    if (c_.has_mtp) {   // code_pred.mtp_proj (1.7B): tts_transformer.cpp:611-616, 709-712
        if (!(mtp_ = up16("code_pred.mtp_proj.weight", H, c_.cp_hidden))) return false;
        if (g.find("code_pred.mtp_proj.bias") && !(mtp_b_ = up32("code_pred.mtp_proj.bias", c_.cp_hidden))) return false;
    }
    if (!(text_embd_ = up16("talker.text_embd.weight", c_.text_dim, c_.text_vocab))) return false;
    if (!(fc1_ = up16("talker.text_proj.fc1.weight", c_.text_dim, c_.text_dim))) return false;
    if (!(fc2_ = up16("talker.text_proj.fc2.weight", c_.text_dim, H))) return false;
    if (!(fc1_b_ = up32("talker.text_proj.fc1.bias", c_.text_dim))) return false;
    if (!(fc2_b_ = up32("talker.text_proj.fc2.bias", H))) return false;
    if (!(codec_embd_ = up16("talker.codec_embd.weight", H, c_.codec_vocab))) return false;
    if (!(codec_head_ = up16("talker.codec_head.weight", H, c_.codec_vocab))) return false;
    if (!(out_norm_ = up32("talker.output_norm.weight", H))) return false;
    if (!(cp_out_norm_ = up32("code_pred.output_norm.weight", c_.cp_hidden))) return false;
    cp_embd_.resize(15);
    cp_head_.resize(15);
    for (int i = 0; i < 15; ++i) {
        char b[96];
        snprintf(b, sizeof b, "code_pred.codec_embd.%d.weight", i);
        if (!(cp_embd_[i] = up16(b, H, c_.cp_vocab))) return false;
        snprintf(b, sizeof b, "code_pred.lm_head.%d.weight", i);
        if (!(cp_head_[i] = up16(b, c_.cp_hidden, c_.cp_vocab))) return false;
    }
    // speaker encoder (ECAPA-TDNN, audio_tokenizer_encoder.cpp): optional, the GGUF's spk_enc.* tensors
    if (g.find("spk_enc.conv0.weight")) {
        spk_.reset(new SpeakerEncoder());
        if (!spk_->load(g, wa_, stream_)) return false;
    }
    return true;
}

// the weight arena of a model file laid out on the host only (WeightArena::plan): the offsets of every allocation in
// order and the bytes used -- what every rank of a shared start-up computes from the GGUF headers before the RCCL
// broadcast (comm_bcast_arenas checks the sizes; tests/test_dist_cpu.py compares whole layouts across gloo ranks)
bool Engine::plan_layout(const std::string &tts_gguf, std::vector<size_t> &offsets, size_t &used) {
    Gguf g;
    if (!g.open(tts_gguf)) { set_error(g.error()); return false; }
    if (!parse_config(g)) return false;
    wa_.plan = wa_.recv = true;
    wa_.trace = &offsets;
    const bool ok = layout_weights(g);
    wa_.trace = nullptr;
    used = wa_.used;
    return ok;
}

bool Engine::upload_weights_rest() {
    const int D = c_.head_dim;
    // the 16 tables of the step embedding: codec_embd (code 0) + code_pred.codec_embd[0..14] (codes 1..15)
    std::vector<uint16_t *> tabs16(16);
    tabs16[0] = codec_embd_;
    for (int i = 0; i < 15; ++i) tabs16[1 + i] = cp_embd_[i];
    tabs16_dev_ = dalloc<uint16_t *>(16);
    Q3T_HIP(hipMemcpyAsync(tabs16_dev_, tabs16.data(), 16 * sizeof(uint16_t *), hipMemcpyHostToDevice, stream_));
    Q3T_HIP(hipStreamSynchronize(stream_));
    // RoPE cos/sin table with ggml_rope_cache_init's f32 recurrence (theta *= theta_scale), NEOX pairs
    rope_len_ = std::max(max_ctx_, 16);
    std::vector<float> rope((size_t)rope_len_ * D);
    const float theta_scale = powf(c_.rope_theta, -2.0f / (float)D);
    for (int p = 0; p < rope_len_; ++p) {
        float theta = (float)p;
        for (int i0 = 0; i0 < D; i0 += 2) {
            rope[(size_t)p * D + i0] = cosf(theta);
            rope[(size_t)p * D + i0 + 1] = sinf(theta);
            theta *= theta_scale;
        }
    }
    rope_ = dalloc<float>(rope.size());
    Q3T_HIP(hipMemcpyAsync(rope_, rope.data(), rope.size() * 4, hipMemcpyHostToDevice, stream_));
    Q3T_HIP(hipStreamSynchronize(stream_));
    return true;
}

bool Engine::alloc_state() {
    const int S = max_slots_, H = c_.hidden, D = c_.head_dim;
    const int QKV = std::max(c_.n_heads + 2 * c_.n_kv, c_.cp_heads + 2 * c_.cp_kv) * D;   // talker / code predictor
    max_trailing_ = 512;
    x_ = dalloc<float>((size_t)S * H);
    qkv_ = dalloc<float>((size_t)S * QKV);
    logits_ = dalloc<float>((size_t)S * c_.codec_vocab);
    hidden_ = dalloc<float>((size_t)S * H);
    cpx_ = dalloc<float>((size_t)S * c_.cp_hidden);
    cp_in1_ = dalloc<float>((size_t)S * H);
    if (c_.has_mtp) mtp_in_ = dalloc<uint16_t>((size_t)S * H);
    cp_logits_ = dalloc<float>((size_t)S * c_.cp_vocab);
    // (the code-predictor stack runs attn_decode on these too: sized for the wider of the two head layouts)
    part_ = dalloc<float>((size_t)S * std::max(c_.n_heads, c_.cp_heads) * talker_cache().max_splits * (D + 2));
    ticket_ = dalloc<unsigned>((size_t)S * std::max(c_.n_kv, c_.cp_kv));
    sel_ticket_ = dalloc<unsigned>((size_t)S);
    attn_ = dalloc<uint16_t>((size_t)S * std::max(c_.n_heads, c_.cp_heads) * D);
    hmlp_ = dalloc<uint16_t>((size_t)S * std::max(c_.inter, c_.cp_inter));
    xn_ = dalloc<uint16_t>((size_t)S * H);
    parts_ = dalloc<float>((size_t)4 * S * H);
    const size_t kv_layer = talker_cache().kv_layer, cpkv_layer = cp_cache(0).kv_layer;
    kc_ = dalloc<uint16_t>(kv_layer * c_.n_layers);
    vc_ = dalloc<uint16_t>(kv_layer * c_.n_layers);
    cpkc_ = dalloc<uint16_t>(cpkv_layer * c_.cp_layers);
    cpvc_ = dalloc<uint16_t>(cpkv_layer * c_.cp_layers);
    pos_ = dalloc<int>(S);
    frame_ = dalloc<int>(S);
    done_ = dalloc<int>(S);
    token_ = dalloc<int>(S);
    tokens_ = dalloc<int>((size_t)S * 16);
    n_tokens_ = dalloc<int>(S);
    force_ = dalloc<int>(S);
    trailing_len_ = dalloc<int>(S);
    cp_pos_ = dalloc<int>((size_t)16 * S);
    seen_ = dalloc<uint8_t>((size_t)S * c_.codec_vocab);
    utt_ = dalloc<uint64_t>(S);
    seed_dev_ = dalloc<uint64_t>(1);
    slot_iota_ = dalloc<int>(S);
    sel_rec_ = dalloc<SelRec>(S);
    slot_max_len_ = dalloc<int>(S);
    trailing_ = dalloc<float>((size_t)S * max_trailing_ * H);
    tts_pad_ = dalloc<float>((size_t)S * H);
    codes_max_len_ = max_ctx_;
    codes_ = dalloc<int32_t>((size_t)S * codes_max_len_ * 16);
    if (!alloc_prompt_scratch(main_ps_, cp_in1_)) return false;
    if (!x_ || !kc_ || !vc_ || !sel_rec_ || !slot_max_len_) { set_error("device allocation failed"); return false; }
    std::vector<int> cpp((size_t)16 * S);
    for (int p = 0; p < 16; ++p) for (int s = 0; s < S; ++s) cpp[(size_t)p * S + s] = p;
    Q3T_HIP(hipMemcpyAsync(cp_pos_, cpp.data(), cpp.size() * 4, hipMemcpyHostToDevice, stream_));
    Q3T_HIP(hipStreamSynchronize(stream_));
    std::vector<uint64_t> utt(S);
    for (int s = 0; s < S; ++s) utt[s] = (uint64_t)s;
    Q3T_HIP(hipMemcpyAsync(utt_, utt.data(), S * 8, hipMemcpyHostToDevice, stream_));
    Q3T_HIP(hipStreamSynchronize(stream_));
    std::vector<int> iota(S);
    for (int s = 0; s < S; ++s) iota[s] = s;
    Q3T_HIP(hipMemcpyAsync(slot_iota_, iota.data(), S * 4, hipMemcpyHostToDevice, stream_));
    Q3T_HIP(hipStreamSynchronize(stream_));
    return true;
}

// the persistent launches' weight pointer tables, each uploaded once per context: a stack's layers (pl_dev_ / pl_cp_dev_)
bool Engine::upload_layer_table(const std::vector<DevLayer> &layers, PLayerW *&dev) {
    if (dev) return true;
    std::vector<PLayerW> pl(layers.size());
    for (size_t i = 0; i < layers.size(); ++i)
        pl[i] = PLayerW{layers[i].qkv, layers[i].o, layers[i].gu, layers[i].down, layers[i].attn_norm, layers[i].ffn_norm, layers[i].qn, layers[i].kn};
    dev = dalloc<PLayerW>(pl.size());
    if (!dev) { set_error("device allocation failed"); return false; }
    Q3T_HIP(hipMemcpyAsync(dev, pl.data(), pl.size() * sizeof(PLayerW), hipMemcpyHostToDevice, stream_));
    Q3T_HIP(hipStreamSynchronize(stream_));
    return true;
}
// and the code predictor's 15 lm_heads (heads_dev_)
bool Engine::upload_head_table() {
    if (heads_dev_) return true;
    heads_dev_ = dalloc<const uint16_t *>(16);
    if (!heads_dev_) { set_error("device allocation failed"); return false; }
    std::vector<const uint16_t *> hp(cp_head_.begin(), cp_head_.end());
    Q3T_HIP(hipMemcpyAsync(heads_dev_, hp.data(), hp.size() * sizeof(void *), hipMemcpyHostToDevice, stream_));
    Q3T_HIP(hipStreamSynchronize(stream_));
    return true;
}

// the persistent single-slot talker step (persist.hip): layer pointer table + zeroed hand-off state; off when the
// shapes or the device do not match what the kernel is built for (the launch-per-phase graph is used then)
bool Engine::setup_persist(int n_cu) {
    const bool use = persist_ && fused_select_;
    persist_ = use && persist_supported(c_.hidden, c_.n_heads, c_.n_kv, c_.head_dim, c_.inter, c_.codec_vocab, max_ctx_, n_cu);
    // the code-predictor frame needs the 0.6B code-predictor shapes only: the 1.7B one (a 2,048-wide talker) runs it
    // too, on projected table rows (build_cp_proj_table) with a projected pass-0 input
    const bool cp_ok = use && opt_.persist_cp && c_.cp_vocab == 2048 && c_.codec_vocab == 3072 && CP_.size() >= 1 &&
                       CP_.size() <= 32 && cp_head_.size() == 15 && c_.cp_hidden == 1024 && c_.cp_inter == 3072 &&
                       c_.cp_heads == 16 && c_.cp_kv == 8 && c_.head_dim == 128 && n_cu >= 256;
    // every instantiation must fit one workgroup per CU on this device (occupancy query with its LDS request)
    persist_ = persist_ && persist_resident(device_, max_ctx_, cp_ok);
    persist_cp_ = cp_ok && persist_resident_cp(device_);
    cp_roles_ = persist_cp_ && opt_.cp_roles && c_.cp_layers == 5 && persist_cp_roles_resident(device_);
    tk_roles_ = persist_ && opt_.tk_roles && persist_chunk(max_ctx_) == 64 && persist_tk_roles_supported(max_ctx_) &&
                persist_tk_roles_resident(device_, max_ctx_);
    if (!persist_ && !persist_cp_) return wa_.recv || build_persist_tables();   // (the batched path's table)
    pstate_ = dalloc<uint8_t>(persist_state_bytes());
    if (!pstate_) { set_error("device allocation failed"); return false; }
    if (persist_ && !upload_layer_table(L_, pl_dev_)) return false;
    // the code-predictor frame (persist_cp_frame): its 5 layers and 15 lm_heads
    if (persist_cp_) {
        if (!upload_layer_table(CP_, pl_cp_dev_) || !upload_head_table()) return false;
        // the per-token tables are computed from the weights: a receiving context (replica, non-root rank) builds
        // them once its arena has been filled (finish_weights, after copy_weights_from / the RCCL broadcast)
        if (!wa_.recv && !build_persist_tables()) return false;
    }
    // (pstate_ was zeroed on the context stream by dalloc)
    return true;
}

// the batched code-predictor frame (persist_cpb.hip): the 0.6B code-predictor shapes on the matrix-core family, with
// layer 0 of passes 1..15 from the per-token QKV table (as decoder_stack_mm reads it), on a device that holds its 256
// workgroups at one per CU
bool Engine::setup_cpb(int n_cu) {
    cpb_ = opt_.cpb && mm_ok_ && max_slots_ > 1 && opt_.mm_cp_table && opt_.cp_qkv_table && !c_.has_mtp &&
           c_.cp_vocab == 2048 && c_.codec_vocab == 3072 && CP_.size() == 5 && cp_head_.size() == 15 && cp_embd_.size() >= 14 &&
           c_.cp_hidden == 1024 && c_.hidden == 1024 && c_.cp_inter == 3072 && c_.cp_heads == 16 && c_.cp_kv == 8 &&
           c_.head_dim == 128 && n_cu >= 256 && cpb_resident(device_);
    if (!cpb_) return true;
    cpb_state_ = dalloc<uint8_t>(cpb_state_bytes());
    if (!cpb_state_) { set_error("device allocation failed"); return false; }
    return upload_layer_table(CP_, pl_cp_dev_) && upload_head_table();
}
// the batched talker step (persist_tkb.hip): the 0.6B talker shapes on the matrix-core family, on a device that holds its
// 256 workgroups at one per CU
bool Engine::setup_tkb(int n_cu) {
    tkb_ = opt_.tkb && mm_ok_ && max_slots_ > 1 && !c_.has_mtp && c_.n_layers == 28 && c_.hidden == 1024 &&
           c_.n_heads == 16 && c_.n_kv == 8 && c_.head_dim == 128 && c_.inter == 3072 && c_.codec_vocab == 3072 &&
           n_cu >= 256 && tkb_resident(device_);
    if (!tkb_) return true;
    tkb_state_ = dalloc<uint8_t>(tkb_state_bytes());
    if (!tkb_state_) { set_error("device allocation failed"); return false; }
    return upload_layer_table(L_, pl_dev_);
}
// the slot counts the step serves: the per-op family it reproduces (decoder_stack_mm with k_attn_seq: >= 16 policy
// slots, no forced split attention; split-K 4 for every S_main of these shapes)
bool Engine::use_tkb(int S) const {
    const int S_main = policy_slots_ > 0 ? policy_slots_ : S;
    return tkb_ && use_mm(S) && S <= 64 && S_main >= 16 && S_main <= 64 && !opt_.attn_split;
}
// the slot counts the frame serves: the matrix-core family (decoder_stack_mm) with the split-K of <= 64 slots
bool Engine::use_cpb(int S) const {
    const int S_main = policy_slots_ > 0 ? policy_slots_ : S;
    return cpb_ && cp_qkvtab_ && use_mm(S) && S <= 64 && S_main <= 64;
}

// The code predictor's per-token tables (the layer-0 QKV rows, 520 MB of f32; 1.7B: the projected pass inputs, 130 MB)
// are functions of the weights alone.  One copy per device serves every context that loaded the same weight file
// (path, size and modification time: replicas and test contexts of one model), built by the first of them on its own
// stream and freed with the last one's destruction -- no per-context copy, and no free outside context destruction:
// hipFree synchronises the whole device, and a free while other contexts' threads capture graphs invalidated those
// captures (round 4).
struct CpTables {
    int device = -1;
    std::string key;
    float *qkv = nullptr, *proj = nullptr;
    size_t bytes = 0;
    bool built = false;
    std::mutex build;   // held by the building context; later users wait for the finished tables
    // drop whatever a failed build allocated, so the next context with the same key starts from scratch (no leaked HBM,
    // no bytes counted twice)
    void reset() {
        int prev = -1;
        hipGetDevice(&prev);
        if (device >= 0) hipSetDevice(device);
        if (qkv) hipFree(qkv);
        if (proj) hipFree(proj);
        qkv = proj = nullptr;
        bytes = 0;
        if (prev >= 0) hipSetDevice(prev);   // the caller's current device is restored
    }
    ~CpTables() { reset(); }
};
namespace {
std::mutex g_cp_tables_m;
std::vector<std::weak_ptr<CpTables>> g_cp_tables;
std::shared_ptr<CpTables> cp_tables_for(int device, const std::string &key) {
    std::lock_guard<std::mutex> g(g_cp_tables_m);
    for (auto it = g_cp_tables.begin(); it != g_cp_tables.end();) {
        if (auto t = it->lock()) {
            if (t->device == device && t->key == key) return t;
            ++it;
        } else {
            it = g_cp_tables.erase(it);
        }
    }
    auto t = std::make_shared<CpTables>();
    t->device = device;
    t->key = key;
    g_cp_tables.push_back(t);
    return t;
}
}  // namespace

size_t cp_tables_live_bytes(int device) {   // development / test accounting
    std::lock_guard<std::mutex> g(g_cp_tables_m);
    size_t b = 0;
    for (auto &w : g_cp_tables)
        if (auto t = w.lock())
            if (t->device == device) b += t->bytes;
    return b;
}

// Built whenever a path reads them: the persistent frame (persist_cp_), or the batched code predictor
// (Q3T_MM_CP_TABLE, 0.6B shapes), so the batched arithmetic depends on the shapes and options, not on whether this
// device runs persistent kernels.
bool Engine::build_persist_tables() {
    if (tables_built_) return true;
    const bool qkv_shapes = opt_.cp_qkv_table && c_.codec_vocab == 3072 && c_.cp_vocab == 2048 && (int)cp_embd_.size() >= 14 &&
                            cpc_.hidden == 1024 && (int)CP_.size() >= 1;
    // (1.7B on the matrix-core stack: the selection hand-offs of passes 1..15 read the projected rows)
    const bool want_proj = c_.has_mtp && (persist_cp_ || (mm_ok_ && max_slots_ > 1));
    const bool want_qkv = qkv_shapes && (persist_cp_ || (opt_.mm_cp_table && mm_ok_ && max_slots_ > 1));
    if (!want_proj && !want_qkv) { tables_built_ = true; return true; }
    struct stat st{};
    if (stat(tts_path_.c_str(), &st) != 0) { set_error("stat failed: " + tts_path_); return false; }
    const std::string key = tts_path_ + "|" + std::to_string((long long)st.st_size) + "|" + std::to_string((long long)st.st_mtime) +
                            (want_proj ? "|proj" : "") + (want_qkv ? "|qkv" : "");
    cp_tables_ = cp_tables_for(device_, key);
    std::lock_guard<std::mutex> g(cp_tables_->build);
    if (!cp_tables_->built) {
        // any failure below leaves the entry empty (not half-built) for the next context of this key
        struct Undo {
            CpTables *t;
            bool armed = true;
            ~Undo() { if (armed) t->reset(); }
        } undo{cp_tables_.get()};
        table_iota_ = dalloc<int>(c_.codec_vocab);
        if (!table_iota_) { set_error("device allocation failed (table token iota)"); return false; }
        std::vector<int> ih(c_.codec_vocab);
        for (int i = 0; i < c_.codec_vocab; ++i) ih[i] = i;
        Q3T_HIP(hipMemcpyAsync(table_iota_, ih.data(), ih.size() * 4, hipMemcpyHostToDevice, stream_));
        Q3T_HIP(hipStreamSynchronize(stream_));
        const int QKV = (cpc_.n_heads + 2 * cpc_.n_kv) * cpc_.head_dim;
        const size_t rows = persist_qkv_table_rows();
        if (want_qkv) {
            if (hipMalloc(&cp_tables_->qkv, rows * QKV * sizeof(float)) != hipSuccess) {
                cp_tables_->qkv = nullptr;
                set_error("device allocation failed (code-predictor QKV table)");
                return false;
            }
            cp_tables_->bytes += rows * QKV * sizeof(float);
        }
        if (want_proj) {
            if (hipMalloc(&cp_tables_->proj, rows * c_.cp_hidden * sizeof(float)) != hipSuccess) {
                cp_tables_->proj = nullptr;
                set_error("device allocation failed (code-predictor projected table)");
                return false;
            }
            cp_tables_->bytes += rows * c_.cp_hidden * sizeof(float);
        }
        cp_qkvtab_ = cp_tables_->qkv;
        cp_projtab_ = cp_tables_->proj;
        if (want_proj && !build_cp_proj_table()) return false;
        if (want_qkv && !build_cp_qkv_table()) return false;
        cp_tables_->built = true;
        undo.armed = false;
    }
    cp_qkvtab_ = cp_tables_->qkv;
    cp_projtab_ = cp_tables_->proj;
    tables_built_ = true;
    return true;
}

bool Engine::finish_weights() {
    DeviceLock lk(false, device_);
    Q3T_HIP(hipSetDevice(device_));
    Q3T_HIP(hipStreamSynchronize(stream_));   // the arena fill (copy or broadcast) ran on this stream
    return build_persist_tables();
}

// Layer 0 of code-predictor passes 1..15 starts from a table row (codec_embd / code_pred.codec_embd[p-2]), so its
// raw QKV row is a function of the token alone: computed here once for every token of the 15 tables with the per-op
// pass-input GEMV (PRO_RMS_G1, the K split of a 1-slot step: family_b = 1), whose arithmetic the persistent frame's
// phase A reproduces bit for bit.  The persistent frame then reads the row instead of running layer 0's norm + QKV
// phase and its all-to-all edge (persist.hip).  520 MB of f32.
bool Engine::build_cp_qkv_table() {
    const int H = cpc_.hidden, QKV = (cpc_.n_heads + 2 * cpc_.n_kv) * cpc_.head_dim;
    const int *iota = table_iota_;
    size_t row0 = 0;
    for (int t = 0; t < 15; ++t) {
        const int V = t == 0 ? c_.codec_vocab : c_.cp_vocab;
        GemvParams g;
        g.W = CP_[0].qkv; g.N = QKV; g.K = H; g.B = V;
        g.pro = PRO_RMS_G1; g.nw = CP_[0].attn_norm; g.eps = c_.eps;
        g.gs.tok = iota; g.gs.tok_ld = 1; g.gs.tok_col0 = 0;
        g.gs.tab0 = t == 0 ? codec_embd_ : cp_embd_[t - 1];
        if (cp_projtab_) {   // 1.7B: layer 0 normalises the projected row (the per-op path's PRO_RMS on cpx_)
            g.pro = PRO_RMS; g.x = cp_projtab_ + row0 * H; g.ldx = H;
        }
        g.out_f32 = cp_qkvtab_ + row0 * QKV; g.ldo = QKV;
        g.family_b = 1;
        if (!gemv(g, stream_)) return false;
        row0 += V;
    }
    Q3T_HIP(hipStreamSynchronize(stream_));
    return true;
}

// 1.7B: every code-predictor pass input is mtp_proj . f16(row) + b of a talker-space row; for passes 1..15 the row is a
// table row, so the projected input is a function of the token: computed once here for the 15 tables with the per-op
// path's own launches (k_gather_sum + the mtp_proj GEMV with a 1-slot K split), the persistent frame then reads it
// (130 MB of f32).
bool Engine::build_cp_proj_table() {
    const int H = c_.hidden, CH = c_.cp_hidden;
    const int *iota = table_iota_;
    // scratch rows: the QKV table's first codec_vocab x H floats when it exists (written after this build), else kept
    float *rowbuf = cp_qkvtab_ ? cp_qkvtab_ : dalloc<float>((size_t)c_.codec_vocab * H);
    if (!cp_projtab_ || !rowbuf) { set_error("device allocation failed (code-predictor projected table)"); return false; }
    size_t row0 = 0;
    for (int t = 0; t < 15; ++t) {
        const int V = t == 0 ? c_.codec_vocab : c_.cp_vocab;
        GatherSum gs;
        gs.tok = iota; gs.tok_ld = 1; gs.tok_col0 = 0;
        gs.tab0 = t == 0 ? codec_embd_ : cp_embd_[t - 1];
        if (!gather_sum(gs, 1, V, H, rowbuf, H, stream_)) return false;
        GemvParams g;
        g.W = mtp_; g.N = CH; g.K = H; g.B = V;
        g.pro = PRO_F32; g.x = rowbuf; g.ldx = H;
        g.bias = mtp_b_;
        g.out_f32 = cp_projtab_ + row0 * CH; g.ldo = CH; g.family_b = 1;
        if (!gemv(g, stream_)) return false;
        row0 += V;
    }
    Q3T_HIP(hipStreamSynchronize(stream_));
    return true;
}

bool Engine::persist_recover() {
    Q3T_HIP(hipStreamSynchronize(stream_));
    fprintf(stderr, "[q3t] persistent kernel flagged an in-launch hand-off fault on device %d: "
                    "falling back to the launch-per-op graphs for this context\n", device_);
    if (pstate_) Q3T_HIP(hipMemsetAsync(pstate_, 0, persist_state_bytes(), stream_));   // ordered before the re-run on stream_
    if (cpb_state_ && !cpb_clear(cpb_state_, stream_)) return false;
    if (tkb_state_ && !tkb_clear(tkb_state_, stream_)) return false;
    Q3T_HIP(hipStreamSynchronize(stream_));
    for (auto &kv : g_talker_) hipGraphExecDestroy(kv.second);
    for (auto &kv : g_frame_) hipGraphExecDestroy(kv.second);
    for (auto &kv : g_cp_) hipGraphExecDestroy(kv.second);
    g_talker_.clear(); g_frame_.clear(); g_cp_.clear();
    persist_ = persist_cp_ = cp_roles_ = tk_roles_ = cpb_ = tkb_ = false;
    // the tables (serving only the persistent frame) stay allocated until the context is destroyed: a hipFree here
    // would synchronise the device and invalidate graph captures other contexts' threads have in progress
    // the per-op code predictor with its attention as its own launch reproduces the persistent frame bit for bit
    // (as does the per-op talker step for n_ctx <= 2048), so a re-run regenerates the frames already delivered exactly
    cp_fused_attn_ = false;
    persist_fallback_ = true;
    return true;
}

#ifdef Q3T_DEV
bool Engine::debug_read(int which, void *dst, size_t bytes) {
    if (which == 5 && pprof_) {   // persistent-step timeline (dev)
        Q3T_HIP(hipStreamSynchronize(stream_));
        Q3T_HIP(hipMemcpy(dst, pprof_, std::min<size_t>(bytes, (size_t)PROF_WG * PROF_PH * 4 * 8), hipMemcpyDeviceToHost));
        return true;
    }
    if (which == 4 && !pstate_) {   // launch-per-phase attention partial buffer (dev dumps)
        Q3T_HIP(hipStreamSynchronize(stream_));
        Q3T_HIP(hipMemcpy(dst, part_, std::min<size_t>(bytes, (size_t)max_slots_ * c_.n_heads * talker_cache().max_splits * (c_.head_dim + 2) * 4), hipMemcpyDeviceToHost));
        return true;
    }
    if (which == 4 && pstate_) {   // persistent-step partial buffer (dev dumps)
        PersistParams pp;
        persist_carve(pstate_, pp);
        Q3T_HIP(hipStreamSynchronize(stream_));
        Q3T_HIP(hipMemcpy(dst, pp.part, std::min<size_t>(bytes, 8 * 32 * 2 * 130 * 4), hipMemcpyDeviceToHost));
        return true;
    }
    const void *src = which == 0 ? (const void *)kc_ : which == 1 ? (const void *)vc_ : which == 2 ? (const void *)qkv_ : (const void *)attn_;
    const size_t kvb = (size_t)max_slots_ * c_.n_kv * max_ctx_ * c_.head_dim * c_.n_layers * 2;
    const size_t cap = which <= 1 ? kvb : which == 2 ? (size_t)max_slots_ * (c_.n_heads + 2 * c_.n_kv) * c_.head_dim * 4
                                                     : (size_t)max_slots_ * c_.n_heads * c_.head_dim * 2;
    if (which < 0 || which > 3 || bytes > cap) { set_error("debug_read: bad buffer or size"); return false; }
    Q3T_HIP(hipStreamSynchronize(stream_));
    Q3T_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return true;
}
#endif

// test hook (Q3T_PERSIST_FAULT_AT=n): the graph replay that contains the n-th persistent launch of this context runs
// with the abort word already set, exactly as if one of its hand-off waits had given up.  Host-side on purpose: a
// device-side launch counter in k_persist's prologue cost 32 us per talker step in code generation alone.
bool Engine::persist_fault_hook(int S, int n_launches) {
    if (!opt_.persist_fault_at || S != 1 || !persist_enabled() || !pstate_) return true;
    const unsigned before = persist_launches_;
    persist_launches_ += (unsigned)n_launches;
    if (before < opt_.persist_fault_at && opt_.persist_fault_at <= persist_launches_) {
        PersistParams p;
        persist_carve(pstate_, p);
        Q3T_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p.err), 1, 1, stream_));
    }
    return true;
}

bool Engine::persist_error() {
    if (cpb_ && cpb_state_) {
        bool e = false;
        if (!cpb_error(cpb_state_, stream_, &e) || e) return true;
    }
    if (tkb_ && tkb_state_) {
        bool e = false;
        if (!tkb_error(tkb_state_, stream_, &e) || e) return true;
    }
    if (!(persist_ || persist_cp_) || !pstate_) return false;
    PersistParams p;
    persist_carve(pstate_, p);
    // on the context's own (non-blocking) stream: a null-stream copy would order against, and break, graph captures
    // in progress on other threads' streams
    unsigned e = 0;
    if (hipMemcpyAsync(&e, p.err, 4, hipMemcpyDeviceToHost, stream_) != hipSuccess || hipStreamSynchronize(stream_) != hipSuccess)
        return true;
    return e != 0;
}

struct StackInput {
    int pro = PRO_RMS;
    bool prenormed = false;              // batched: x / xn already hold layer 0's input (select_embed_norm)
    const float *x = nullptr;
    GatherSum gs;
    SelectSpec sel;                      // PRO_SEL_G1: selection of the gathered token
    const float *sel_logits = nullptr;
};
// one run of a decoder stack: where it computes, the cache it attends over and the per-call choices
struct StackRun {
    StackBufs buf;
    StackCache kv;
    const StackInput *in0 = nullptr;     // replaces layer 0's activation source (null: buf.x as it stands)
    // the batch whose kernel choices this run reproduces, 0: its own S (a continuous-batching admission runs ONE slot
    // and the causal prefill its rows with the kernels and K split of the batch, so the per-token arithmetic is the
    // batch's)
    int family = 0;
    const PrefillAttnParams *pf = nullptr;   // the causal prefill's attention in place of the decode launch
    bool cp_attn = false;                // matrix-core stack: the code predictor's (k_attn_small, no weight prefetch)
    bool fused_cp_attn = false;          // vector stack: that attention recomputed inside the O-projection prologue
    // matrix-core stack: the norm after the last layer (null: none, code-predictor pass 0 has no head), its f32 side
    // output, and layer 0's raw QKV rows from the per-token table (the tab_* fields) in place of its QKV GEMM
    const float *final_norm = nullptr;
    float *final_side = nullptr;
    AttnParams l0tab;                    // (only its qkv_tab / tab_* fields are read)
};
struct MmAttn { int seqk, small; bool l0tab; };   // the matrix-core stack's attention kernel choices

// layer il's attention of either stack body: the decode launch over each slot's new token, or the causal prefill's
// (r.pf) over layer il's cache and the stack's activations
static bool stack_attn(const Config &c, const DevLayer &l, size_t il, int S, const StackRun &r, const MmAttn *mm, hipStream_t s) {
    uint16_t *kc = r.kv.kc + il * r.kv.kv_layer, *vc = r.kv.vc + il * r.kv.kv_layer;
    if (r.pf) {
        PrefillAttnParams q = *r.pf;
        q.qkv = r.buf.qkv; q.qn = l.qn; q.kn = l.kn; q.eps = c.eps; q.rope = r.kv.rope; q.kc = kc; q.vc = vc;
        q.n_ctx = r.kv.n_ctx; q.nH = c.n_heads; q.nKV = c.n_kv; q.D = c.head_dim; q.out = r.buf.attn;
        return prefill_attn(q, s);
    }
    AttnParams a = mm && mm->l0tab && il == 0 ? r.l0tab : AttnParams();
    a.qkv = r.buf.qkv; a.qn = l.qn; a.kn = l.kn; a.eps = c.eps; a.rope = r.kv.rope; a.pos = r.kv.pos; a.kc = kc; a.vc = vc;
    a.n_ctx = r.kv.n_ctx; a.S = S; a.nH = c.n_heads; a.nKV = c.n_kv; a.D = c.head_dim;
    a.max_splits = r.kv.max_splits;   // chunk 128 measured no faster at 64 slots (1.79 vs 1.77 ms per step)
    a.part = r.kv.part; a.ticket = r.kv.ticket; a.out = r.buf.attn;
    if (mm) { a.seqk = mm->seqk; a.small = mm->small; }
#ifdef Q3T_DEV
    if (!mm && il == 0 && std::getenv("Q3T_PERSIST_DBG")) a.dbg = r.kv.part;
#endif
    return attn_decode(a, s);
}

// final RMSNorm + head GEMV -> logits.  h names the head: W, N, out_f32, force_mm, and for the vector form (the norm in
// the GEMV's prologue, over b.x) the norm weight nw, the normalised rows' side_out, family_b and a fused selection.
// hoisted: the matrix-core stack's last resid_norm already normalised the rows into b.xn (and wrote its side output)
static bool head_gemv(const Config &c, GemvParams h, const StackBufs &b, bool hoisted, int S, hipStream_t s) {
    h.K = c.hidden; h.B = S; h.ldx = c.hidden; h.ldo = h.N; h.eps = c.eps;
    h.pro = hoisted ? PRO_F16 : PRO_RMS;
    h.x = hoisted ? (const void *)b.xn : b.x;
    if (hoisted) { h.nw = nullptr; h.side_out = nullptr; h.family_b = 0; h.sel = SelectSpec(); }
    return gemv(h, s);
}

// ------------------------------------------------------------------------------------------ batched decoder stack
// matrix-core path (S >= gemm_mfma_min_batch()): 7 launches per layer so that every projection fills the chip:
//   [QKV GEMM on xn] [attention] [O GEMM, split-K slabs] [resid + RMSNorm(ffn) -> xn] [gate/up GEMM + SwiGLU]
//   [down GEMM, split-K slabs] [resid + RMSNorm(next attn_norm | final norm) -> xn]
// The norms are hoisted out of the GEMM prologues (each projection workgroup used to recompute the norm of its
// tokens: ~12 us of chained double math per launch at 64 slots) and the N = 1024 projections split K four ways
// (32 row tiles x 2 token tiles would leave 192 of 256 CUs idle).  final_norm null: no normalisation after the last
// layer (code-predictor pass 0 has no head).
static int splitk_for(int N, int S, int K) {
    const int tiles = (N / 32) * ((S + 31) / 32), nch = K / 256;
    // K chunks per slice must be one of the GEMM kernel's instantiations (gemm_mfma_supported)
    auto ok = [&](int ks) { const int nk = nch % ks == 0 ? nch / ks : 0; return nk == 1 || nk == 2 || nk == 3 || nk == 4 || nk == 8 || nk == 12; };
    for (int ks : {1, 2, 3, 4})
        if (ok(ks) && tiles * ks >= 256) return ks;
    for (int ks : {4, 3, 2})
        if (ok(ks)) return ks;
    return 1;
}
static bool decoder_stack_mm(const Config &c, const Options &opt, const std::vector<DevLayer> &layers, int S, const StackRun &r,
                             hipStream_t s) {
    float *const x = r.buf.x, *const parts = r.buf.parts, *const qkv = r.buf.qkv;
    uint16_t *const xn = r.buf.xn, *const attn = r.buf.attn, *const hmlp = r.buf.hmlp;
    const int S_main = r.family > 0 ? r.family : S;
    const bool force = S < gemm_mfma_min_batch();
    const int H = c.hidden, D = c.head_dim, QKV = (c.n_heads + 2 * c.n_kv) * D;
    ResidNorm rn;
    rn.S = S; rn.H = H; rn.eps = c.eps; rn.x = x; rn.xn = xn;
    rn.nw = layers[0].attn_norm;
    const bool gathered = r.in0 && (r.in0->pro == PRO_RMS_G1 || r.in0->pro == PRO_RMS_G16);
    if (r.in0 && !gathered) rn.xin = r.in0->x;   // copied into the residual stream by the norm
    // prenormed: the previous launch (token selection) gathered and normalised layer 0's input
    if (!(r.in0 && r.in0->prenormed)) {
        if (gathered && !gather_sum(r.in0->gs, r.in0->pro == PRO_RMS_G16 ? 16 : 1, S, H, x, H, s)) return false;
        if (!resid_norm(rn, s)) return false;
    }
    rn.xin = nullptr;
    // the code predictor's <= 16 positions run on k_attn_small, which can read layer 0's raw QKV rows from the per-token
    // table (l0tab: passes 1..15) instead of a QKV GEMM over xn (one wave per (slot, kv head), the 0.6B head layout);
    // k_attn_seq once there are enough (slot, kv head) pairs to fill the chip
    const bool small = r.cp_attn && r.kv.n_ctx <= 16 && D == 128 && c.n_heads == 2 * c.n_kv;
    const bool use_tab = small && r.l0tab.qkv_tab && !r.pf;
    const MmAttn am{S_main >= 16 && !opt.attn_split, small, use_tab};
    for (size_t il = 0; il < layers.size(); ++il) {
        const DevLayer &l = layers[il];
        GemvParams g;
        g.W = l.qkv; g.N = QKV; g.K = H; g.B = S;
        g.pro = PRO_F16; g.x = xn; g.ldx = H;
        g.out_f32 = qkv; g.ldo = QKV; g.force_mm = force;
        if (!(il == 0 && use_tab) && !gemv(g, s)) return false;
        if (!stack_attn(c, l, il, S, r, &am, s)) return false;
        // code-predictor pass 0 (no head): its last layer's K/V rows, appended above, are all that is ever read
        if (il + 1 == layers.size() && !r.final_norm) break;
        GemvParams o;
        o.W = l.o; o.N = H; o.K = c.n_heads * D; o.B = S;
        o.pro = PRO_F16; o.x = attn; o.ldx = c.n_heads * D;
        o.parts = parts; o.ksplit = splitk_for(H, S_main, o.K); o.force_mm = force;
        if (!gemv(o, s)) return false;
        rn.parts = parts; rn.ksplit = o.ksplit; rn.nw = l.ffn_norm; rn.side = nullptr;
        // the talker's weights stream from HBM each step: the norm before a projection touches that projection's lines
        // (the code predictor's 157 MB stay in the Infinity Cache across its 16 passes anyway)
        const bool pf_w = !r.cp_attn && opt.mm_prefetch > 0;
        rn.prefetch = pf_w ? l.gu : nullptr; rn.prefetch_bytes = (size_t)2 * c.inter * H * 2;
        if (!resid_norm(rn, s)) return false;
        GemvParams gu;
        gu.W = l.gu; gu.N = 2 * c.inter; gu.K = H; gu.B = S;
        gu.pro = PRO_F16; gu.x = xn; gu.ldx = H;
        gu.act = ACT_SWIGLU; gu.out_f16 = hmlp; gu.ldo = c.inter; gu.force_mm = force; gu.mm_tt = opt.mm_gu_tt;
        if (pf_w && opt.mm_prefetch > 1) { gu.prefetch = l.down; gu.prefetch_bytes = (size_t)c.inter * H * 2; }
        if (!gemv(gu, s)) return false;
        GemvParams dn;
        dn.W = l.down; dn.N = H; dn.K = c.inter; dn.B = S;
        dn.pro = PRO_F16; dn.x = hmlp; dn.ldx = c.inter;
        dn.parts = parts; dn.ksplit = splitk_for(H, S_main, dn.K); dn.force_mm = force;
        dn.xcd_slices = true;   // each XCD fetches 1 / ksplit of hmlp (FETCH 1.42x -> 1.06x of the algorithmic bytes)
        if (!gemv(dn, s)) return false;
        const bool last = il + 1 == layers.size();
        if (last && !r.final_norm) break;   // code-predictor pass 0: only its K/V caches are read afterwards
        rn.parts = parts; rn.ksplit = dn.ksplit;
        rn.nw = last ? (r.final_norm ? r.final_norm : l.ffn_norm) : layers[il + 1].attn_norm;
        rn.side = last ? r.final_side : nullptr;
        rn.prefetch = pf_w && !last ? layers[il + 1].qkv : nullptr; rn.prefetch_bytes = (size_t)QKV * H * 2;
        if (!resid_norm(rn, s)) return false;
        rn.prefetch = nullptr;
    }
    return true;
}

// ------------------------------------------------------------------------------------------ one decoder stack
// 5 launches per layer: [RMSNorm+QKV GEMV] [head-norm+RoPE+KV-append+attention] [O GEMV + residual]
// [RMSNorm+gate/up GEMV+SwiGLU] [down GEMV + residual]   (tts_transformer.cpp:1410-1494)
// `r.in0` (optional) replaces layer 0's activation source: a gather prologue or another f32 buffer, with the raw
// rows written to x (the residual stream) by the QKV kernel itself.

static bool decoder_stack(const Config &c, const std::vector<DevLayer> &layers, int S, const StackRun &r, hipStream_t s) {
    // r.pf: the causal prefill (S = its rows, run with the vector kernels of a family_b-slot step)
    float *const x = r.buf.x, *const qkv = r.buf.qkv;
    uint16_t *const attn = r.buf.attn, *const hmlp = r.buf.hmlp;
    const int H = c.hidden, D = c.head_dim, QKV = (c.n_heads + 2 * c.n_kv) * D, family_b = r.family;
    // batched (matrix-core) path: gathers become their own launch and the code predictor's attention runs unfused
    const bool mm = (family_b > 0 ? family_b : S) >= gemm_mfma_min_batch();
    const bool fused_cp_attn = r.fused_cp_attn && !mm && !r.pf;
    for (size_t il = 0; il < layers.size(); ++il) {
        const DevLayer &l = layers[il];
        GemvParams g;
        g.W = l.qkv; g.N = QKV; g.K = H; g.B = S;
        g.pro = PRO_RMS; g.x = x; g.ldx = H; g.nw = l.attn_norm; g.eps = c.eps;
        if (il == 0 && r.in0) {
            // the gather as its own launch: batched path (no gather prologue in the GEMM), or rows wider than the
            // GEMV's gather prologue (K > 1024: the 1.7B talker) -- the same summation order either way
            if ((mm || H > 1024) && (r.in0->pro == PRO_RMS_G1 || r.in0->pro == PRO_RMS_G16)) {
                if (!gather_sum(r.in0->gs, r.in0->pro == PRO_RMS_G16 ? 16 : 1, S, H, x, H, s)) return false;
            } else {
                g.pro = r.in0->pro; g.x = r.in0->x; g.gs = r.in0->gs; g.raw_out = x;
                g.sel = r.in0->sel; g.sel_logits = r.in0->sel_logits;
            }
        }
        g.out_f32 = qkv; g.ldo = QKV; g.family_b = family_b;
        if (!gemv(g, s)) return false;
        GemvParams o;
        o.W = l.o; o.N = H; o.K = c.n_heads * D; o.B = S; o.family_b = family_b;
        if (fused_cp_attn) {
            // code predictor: attention recomputed inside the O-projection prologue (<= 16 positions)
            o.pro = PRO_CPATT;
            o.att.qkv = qkv; o.att.ld = QKV; o.att.qn = l.qn; o.att.kn = l.kn; o.att.eps = c.eps;
            o.att.rope = r.kv.rope; o.att.pos = r.kv.pos;
            o.att.kc = r.kv.kc + il * r.kv.kv_layer; o.att.vc = r.kv.vc + il * r.kv.kv_layer;
        } else {
            if (!stack_attn(c, l, il, S, r, nullptr, s)) return false;
            o.pro = PRO_F16; o.x = attn; o.ldx = c.n_heads * D;
        }
        o.resid = x; o.ldr = H; o.out_f32 = x; o.ldo = H;
        if (!gemv(o, s)) return false;
        GemvParams gu;
        gu.W = l.gu; gu.N = 2 * c.inter; gu.K = H; gu.B = S;
        gu.pro = PRO_RMS; gu.x = x; gu.ldx = H; gu.nw = l.ffn_norm; gu.eps = c.eps;
        gu.act = ACT_SWIGLU; gu.out_f16 = hmlp; gu.ldo = c.inter; gu.family_b = family_b;
        if (!gemv(gu, s)) return false;
        GemvParams dn;
        dn.W = l.down; dn.N = H; dn.K = c.inter; dn.B = S; dn.family_b = family_b;
        dn.pro = PRO_F16; dn.x = hmlp; dn.ldx = c.inter;
        dn.resid = x; dn.ldr = H; dn.out_f32 = x; dn.ldo = H;
        if (!gemv(dn, s)) return false;
    }
    return true;
}

bool Engine::enqueue_talker_step(int S, hipStream_t s) { return enqueue_talker(S, s, false, false); }

SelectSpec Engine::select_spec(int mode, const GenParams &gp, int frame_offset, int step) const {
    SelectSpec sp;
    sp.mode = mode;
    sp.V = mode == SEL_CB0 ? c_.codec_vocab : c_.cp_vocab;
    sp.ticket = sel_ticket_;
    sp.tokens = tokens_; sp.codes = codes_; sp.max_len = codes_max_len_; sp.ncb = 16;
    sp.frame = frame_; sp.frame_offset = frame_offset; sp.done = done_;
    sp.temperature = gp.temperature; sp.top_k = gp.top_k; sp.seed = gp.seed; sp.seed_dev = seed_dev_; sp.utt = utt_;
    sp.step = step;
    sp.seen = seen_; sp.n_tokens = n_tokens_; sp.force_frames = force_; sp.eos = c_.codec_eos; sp.rep = gp.rep_penalty;
    if (rec_on_) sp.rec = sel_rec_;   // per-utterance sampling: the slots' records in place of the scalars
    return sp;
}

// gather_input: the step embedding (tts_transformer.cpp:2529-2553) is assembled by layer 0's QKV prologue from the
// frame's 16 codes (PRO_RMS_G16) instead of being read from x_
// select_next: the codec head's last workgroup also selects CB0 of the NEXT frame (frame_ + 1) in the same launch
bool Engine::enqueue_talker(int S, hipStream_t s, bool gather_input, bool select_next, bool prenormed, bool *fold_advance) {
    if (S == 1 && persist_) return talker_persist_one(s, gather_input, select_next, fold_advance);
    if (use_tkb(S)) return talker_persist_batched(S, s, gather_input && !prenormed, select_next);
    return talker_per_op(S, s, gather_input, select_next, prenormed);
}

StackCache Engine::talker_cache() const {
    return {kc_, vc_, (size_t)max_slots_ * c_.n_kv * max_ctx_ * c_.head_dim, max_ctx_, (max_ctx_ + ATTN_CHUNK - 1) / ATTN_CHUNK, pos_, rope_, part_, ticket_};
}
// pass p's position is p for every slot (cp_pos_ rows); its 16 positions are one attention chunk
StackCache Engine::cp_cache(int p) const {
    return {cpkc_, cpvc_, (size_t)max_slots_ * cpc_.n_kv * 16 * cpc_.head_dim, 16, 1, cp_pos_ + (size_t)p * max_slots_, rope_, part_, ticket_};
}

GatherSum Engine::step_embed_gather() const {
    GatherSum gs;
    gs.tok = tokens_; gs.tok_ld = 16; gs.tabs = tabs16_dev_;
    gs.tr = trailing_; gs.tr_len = trailing_len_; gs.frame = frame_;
    gs.tr_ld = max_trailing_ * c_.hidden; gs.pad = tts_pad_;
    return gs;
}

// the one-slot step as one persistent launch (persist.hip / persist_tk.hip)
bool Engine::talker_persist_one(hipStream_t s, bool gather_input, bool select_next, bool *fold_advance) {
    const StackCache kv = talker_cache();
    PersistParams p;
    persist_carve(pstate_, p);
    p.L = pl_dev_; p.n_layers = c_.n_layers; p.eps = c_.eps;
    p.gather = gather_input ? 1 : 0; p.x_in = x_; p.gs = step_embed_gather();
    p.rope = kv.rope; p.pos = kv.pos; p.kc = kv.kc; p.vc = kv.vc; p.kv_layer = kv.kv_layer; p.n_ctx = kv.n_ctx;
    p.head = codec_head_; p.out_norm = out_norm_; p.hidden = hidden_; p.logits = logits_;
    if (select_next) p.sel = select_spec(SEL_CB0, gp_, 1, 0);
    p.prof = pprof_;
    if (tk_roles_) {
        if (fold_advance && opt_.fold_advance) {
            p.adv_pos = pos_; p.adv_frame = frame_; p.adv_done = done_; *fold_advance = true;
        }
        return persist_tk_roles(p, s);
    }
    return persist_talker_step(p, s);
}

// batched: the whole step as one persistent launch (persist_tkb.hip); gather: x_ does not hold the step embedding yet
bool Engine::talker_persist_batched(int S, hipStream_t s, bool gather, bool select_next) {
    const StackCache kv = talker_cache();
    if (gather && !gather_sum(step_embed_gather(), 16, S, c_.hidden, x_, c_.hidden, s)) return false;
    TkbParams p;
    p.L = pl_dev_; p.n_layers = c_.n_layers; p.head = codec_head_; p.out_norm = out_norm_;
    p.x_in = x_; p.hidden = hidden_; p.logits = logits_;
    p.rope = kv.rope; p.pos = kv.pos; p.kc = kv.kc; p.vc = kv.vc; p.kv_layer = kv.kv_layer; p.n_ctx = kv.n_ctx;
    if (select_next) { p.select = 1; p.sel = select_spec(SEL_CB0, gp_, 1, 0); }
    p.S = S; p.eps = c_.eps; p.state = tkb_state_; p.prof = pprof_;
    return persist_talker_batched(p, s);
}

bool Engine::talker_per_op(int S, hipStream_t s, bool gather_input, bool select_next, bool prenormed) {
    const bool mm = use_mm(S);   // batched: one selection workgroup per slot after the head
    StackInput in0;
    in0.pro = PRO_RMS_G16; in0.gs = step_embed_gather(); in0.prenormed = prenormed;
    StackRun r;
    r.buf = talker_bufs(); r.kv = talker_cache();
    if (gather_input) r.in0 = &in0;
    r.family = mm ? policy_slots_ : fam1_;
    r.final_norm = out_norm_; r.final_side = hidden_;
    if (mm ? !decoder_stack_mm(c_, opt_, L_, S, r, s) : !decoder_stack(c_, L_, S, r, s)) return false;
    // final RMSNorm (hidden_states, side output) + codec_head -> logits  (:1496-1505)
    GemvParams h;
    h.W = codec_head_; h.N = c_.codec_vocab; h.nw = out_norm_; h.side_out = hidden_; h.out_f32 = logits_; h.family_b = fam1_;
    if (select_next) h.sel = select_spec(SEL_CB0, gp_, 1, 0);
    if (!head_gemv(c_, h, r.buf, mm, S, s)) return false;
    return !(select_next && mm) || select_tokens(h.sel, logits_, S, s);
}

bool Engine::cp_project(int S, const float *x_talker, int ldx, hipStream_t s) {
    GemvParams g;   // ggml_mul_mat(mtp_proj, cur) + ggml_add(bias): f16-rounded input, f32 accumulation
    g.W = mtp_; g.N = c_.cp_hidden; g.K = c_.hidden; g.B = S;
    g.pro = PRO_F32; g.x = x_talker; g.ldx = ldx;
    g.bias = mtp_b_;
    g.out_f32 = cpx_; g.ldo = c_.cp_hidden; g.family_b = fam1_;
    if (use_mm(S)) {
        // matrix-core family: one PRO_F16 GEMM over the f16 of the rows.  Staged in a buffer of its own: the talker's
        // last resid_norm left the same halves in xn_, which the code predictor's stack is about to reuse (and a
        // caller of the frame alone only fills hidden_)
        launch_f32_to_f16(x_talker, mtp_in_, S * c_.hidden, s);
        Q3T_HIP(hipGetLastError());
        g.pro = PRO_F16; g.x = mtp_in_; g.family_b = policy_slots_;
    }
    return gemv(g, s);
}

// 16 passes of the 5-layer code predictor, token chosen on device each pass (trt_code_predictor.cpp:484-600).
// Pass inputs are assembled by layer 0's QKV prologue: pass 0 the talker hidden state, pass 1 codec_embd[code 0],
// pass p >= 2 code_pred.codec_embd[p-2][code p-1]; the raw row lands in cpx_ (the pass's residual stream).
// logits_host (tests only, never captured): every head's logits copied out after its GEMV.
bool Engine::enqueue_cp_frame(int S, hipStream_t s, float *logits_host, bool talker_next) {
    if (S == 1 && persist_cp_ && !logits_host) return cp_frame_persist_one(s);
    if (use_cpb(S) && !logits_host) return cp_frame_persist_batched(S, s, talker_next);
    return cp_frame_per_op(S, s, logits_host, talker_next);
}

// one slot: the whole frame as one persistent launch (persist.hip / persist_cp.hip)
bool Engine::cp_frame_persist_one(hipStream_t s) {
    const StackCache kv = cp_cache(0);
    PersistParams p;
    persist_carve(pstate_, p);
    p.L = pl_cp_dev_; p.n_layers = c_.cp_layers; p.eps = c_.eps; p.x_in = hidden_;
    if (c_.has_mtp) {   // 1.7B: pass 0's projected input by the per-op GEMV, passes 1..15 from the projected table
        if (!cp_project(1, hidden_, c_.hidden, s)) return false;
        p.x_in = cpx_; p.xtab = cp_projtab_;
    }
    p.gs.tok = tokens_; p.gs.tok_ld = 16; p.gs.tabs = tabs16_dev_;
    p.rope = kv.rope; p.kc = kv.kc; p.vc = kv.vc; p.kv_layer = kv.kv_layer; p.n_ctx = kv.n_ctx;
    p.heads = heads_dev_; p.out_norm = cp_out_norm_; p.logits = cp_logits_; p.qkvtab = cp_qkvtab_;
    p.sel = select_spec(SEL_CP, gp_, 0, 0); p.prof = pprof_;
    if (cp_roles_ && p.qkvtab) return persist_cp_roles(p, s);   // (1.7B: layer 0's residual rows from xtab)
    return persist_cp_frame(p, s);
}

// batched: the whole frame as one persistent launch (persist_cpb.hip)
bool Engine::cp_frame_persist_batched(int S, hipStream_t s, bool talker_next) {
    const StackCache kv = cp_cache(0);
    CpbParams p;
    p.L = pl_cp_dev_; p.heads = heads_dev_; p.tabs = tabs16_dev_; p.out_norm = cp_out_norm_; p.qkvtab = cp_qkvtab_;
    p.x_in = hidden_; p.rope = kv.rope; p.pos = kv.pos; p.pos_ld = max_slots_; p.kc = kv.kc; p.vc = kv.vc;
    p.kv_layer = kv.kv_layer; p.logits = cp_logits_; p.sel = select_spec(SEL_CP, gp_, 0, 0); p.S = S; p.eps = c_.eps;
    if (talker_next) {
        const GatherSum gs = step_embed_gather();
        p.talker_next = 1;
        p.tx = x_; p.txn = xn_; p.tnw = L_[0].attn_norm;
        p.tr = gs.tr; p.tr_len = gs.tr_len; p.frame = gs.frame; p.tr_ld = gs.tr_ld; p.pad = gs.pad;
    }
    p.state = cpb_state_; p.prof = pprof_;
    return persist_cp_batched(p, s);
}

// pass p >= 1 starts from the table row of code p - 1: codec_embd for pass 1, code_pred.codec_embd[p - 2] after it
GatherSum Engine::cp_input_gather(int p) const {
    GatherSum gs;
    gs.tok = tokens_; gs.tok_ld = 16; gs.tok_col0 = p - 1; gs.tab0 = p == 1 ? codec_embd_ : cp_embd_[p - 2];
    return gs;
}

// pass p's input: what layer 0 reads (in0), after the launches that prepare it
bool Engine::cp_pass_input(int p, int S, bool defer, StackInput &in0, hipStream_t s) {
    if (c_.has_mtp && use_mm(S)) {
        // 1.7B on the matrix-core stack: pass 0 projects the talker's rows with one GEMM; the projected input of a pass
        // p >= 1 is a function of its token alone, the row of cp_projtab_ (built with the 1-slot GEMV, so independent
        // of the batch) -- gathered here for pass 1 (CB0 was selected by the talker's launch) and by the previous
        // pass's selection hand-off after it (prenormed)
        in0.pro = PRO_RMS; in0.x = cpx_;
        if (p == 0) return cp_project(S, hidden_, c_.hidden, s);
        return in0.prenormed || gather_rows_f32(cp_projtab_, cp_table_row0(p), tokens_, 16, p - 1, S, c_.cp_hidden, cpx_, s);
    }
    if (c_.has_mtp) {
        // 1.7B: the pass input (talker hidden / table row, talker space) projected into cpx_ by code_pred.mtp_proj
        // (tts_transformer.cpp:1554-1560, :1709-1714); layer 0 then normalises cpx_ like any later layer
        if (p > 0 && !gather_sum(cp_input_gather(p), 1, S, c_.hidden, cp_in1_, c_.hidden, s)) return false;
        in0.pro = PRO_RMS; in0.x = cpx_;
        return cp_project(S, p > 0 ? cp_in1_ : hidden_, c_.hidden, s);
    }
    if (p == 0) { in0.pro = PRO_RMS; in0.x = hidden_; return true; }
    in0.pro = PRO_RMS_G1; in0.gs = cp_input_gather(p);
    if (defer && p >= 2) {   // the token of head p - 2 is selected in this pass's QKV launch
        in0.pro = PRO_SEL_G1;
        in0.sel = select_spec(SEL_CP, gp_, 0, p - 2);
        in0.sel_logits = cp_logits_;
    }
    return true;
}

// tests only, never captured: head `step`'s logits of every slot into logits_host [S][15][cp_vocab]
bool Engine::cp_copy_logits(int S, int step, float *logits_host, hipStream_t s) {
    std::vector<float> lg((size_t)S * c_.cp_vocab);
    Q3T_HIP(hipMemcpyAsync(lg.data(), cp_logits_, lg.size() * 4, hipMemcpyDeviceToHost, s));
    Q3T_HIP(hipStreamSynchronize(s));
    for (int b = 0; b < S; ++b)
        std::memcpy(logits_host + ((size_t)b * 15 + step) * c_.cp_vocab, lg.data() + (size_t)b * c_.cp_vocab, c_.cp_vocab * 4);
    return true;
}

// batched: the selecting workgroup of each slot also gathers and normalises the next stage's input (the next pass's
// table row, or the talker step embedding after the last pass)
bool Engine::cp_select_handoff(int S, int step, hipStream_t s) {
    const bool last = step == 14;
    EmbedNorm en;
    en.nt = last ? 16 : 1; en.gs = last ? step_embed_gather() : cp_input_gather(step + 2);
    en.x = last ? x_ : cpx_; en.nw = (last ? L_ : CP_)[0].attn_norm;
    en.xn = xn_; en.eps = c_.eps; en.H = last ? c_.hidden : c_.cp_hidden;
    if (c_.has_mtp && !last) { en.ftab = cp_projtab_; en.ftab_row0 = cp_table_row0(step + 2); }   // the projected row
    return select_embed_norm(select_spec(SEL_CP, gp_, 0, step), cp_logits_, en, S, s);
}

bool Engine::cp_frame_per_op(int S, hipStream_t s, float *logits_host, bool talker_next) {
    const bool mm = use_mm(S);
    // vector path with fused selection: heads 0..13 only produce logits; the next pass's QKV launch selects the token
    // in every workgroup while its weights stream (PRO_SEL_G1), so the head's 256 -> 1 arrival chain and the serial
    // selection leave the critical path.  Head 14 (its token feeds the next talker step) keeps the fused selection.
    const bool fsel_all = fused_select_ && !mm;
    // deferred selection gathers the next pass's table row inside its QKV launch: not with a projected input (1.7B)
    const bool defer = fsel_all && defer_cp_select_ && !c_.has_mtp;
    bool next_prenormed = false;   // batched: this pass's input was prepared by the previous selection launch
    for (int p = 0; p < 16; ++p) {
        StackInput in0;
        in0.prenormed = next_prenormed; next_prenormed = false;
        if (!cp_pass_input(p, S, defer, in0, s)) return false;
        // passes 1..15 of the matrix-core stack: layer 0's raw QKV rows from the per-token table (the 0.6B layout; the
        // table's rows are the 1-slot GEMV's, within the batched family's f32 tolerance of its MFMA GEMM)
        StackRun r;
        if (opt_.mm_cp_table && p >= 1 && cp_qkvtab_) {
            r.l0tab.qkv_tab = cp_qkvtab_; r.l0tab.tab_tok = tokens_; r.l0tab.tab_ld = 16; r.l0tab.tab_col = p - 1;
            r.l0tab.tab_row0 = cp_table_row0(p);
        }
        r.buf = cp_bufs(); r.kv = cp_cache(p);
        if (mm || !c_.has_mtp) r.in0 = &in0;   // (vector stack, 1.7B: layer 0 reads cpx_ like any later layer)
        r.family = mm ? policy_slots_ : fam1_; r.cp_attn = true; r.fused_cp_attn = cp_fused_attn_;
        r.final_norm = p == 0 ? nullptr : cp_out_norm_;
        if (mm ? !decoder_stack_mm(cpc_, opt_, CP_, S, r, s) : !decoder_stack(cpc_, CP_, S, r, s)) return false;
        if (p == 0) continue;
        const int step = p - 1;
        const bool fsel = fsel_all && (!defer || step == 14);
        GemvParams h;
        h.W = cp_head_[step]; h.N = c_.cp_vocab; h.nw = cp_out_norm_; h.out_f32 = cp_logits_; h.family_b = fam1_;
        if (fsel) h.sel = select_spec(SEL_CP, gp_, 0, step);
        if (!head_gemv(cpc_, h, r.buf, mm, S, s)) return false;
        if (logits_host && !cp_copy_logits(S, step, logits_host, s)) return false;
        if (mm && (step < 14 || talker_next)) {
            if (!cp_select_handoff(S, step, s)) return false;
            next_prenormed = true;
        } else if (!fsel && !(defer && step < 14)) {
            if (!select_tokens(select_spec(SEL_CP, gp_, 0, step), cp_logits_, S, s)) return false;
        }
    }
    return true;
}

// one frame = [CB0 select] -> 16 code-predictor passes -> talker step -> pos/frame advance.  With fused selection
// the CB0 of frame f+1 is chosen inside frame f's talker head launch (frame 0's by generate() after the prefill).
bool Engine::enqueue_frame(int S, hipStream_t s) {
    if (!fused_select_ && !select_tokens(select_spec(SEL_CB0, gp_, 0, 0), logits_, S, s)) return false;
    // batched: the last code-predictor selection also assembles and normalises the talker step's input
    const bool mm = use_mm(S);
    if (!enqueue_cp_frame(S, s, nullptr, mm)) return false;
    bool folded = false;   // the single-slot role kernel advances pos / frame itself
    if (!enqueue_talker(S, s, true, fused_select_, mm, &folded)) return false;
    return folded || advance(pos_, frame_, done_, S, s);
}

bool Engine::graph_for(std::map<int, hipGraphExec_t> &cache, int S, bool (Engine::*fn)(int, hipStream_t)) {
    return graph_for_key(cache, S, S, fn);
}

// what `enqueue` launches on stream s, as an executable graph
template <class F>
hipGraphExec_t Engine::capture(hipStream_t s, F &&enqueue) {
    hipGraph_t graph = nullptr;
    hipError_t e = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) { set_error(std::string("graph capture: ") + hipGetErrorString(e)); return nullptr; }
    const bool ok = enqueue();
    e = hipStreamEndCapture(s, &graph);
    if (!ok) { if (graph) hipGraphDestroy(graph); return nullptr; }
    if (e != hipSuccess) { set_error(std::string("graph capture: ") + hipGetErrorString(e)); return nullptr; }
    hipGraphExec_t exec = nullptr;
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    hipGraphDestroy(graph);
    if (e != hipSuccess) { set_error(std::string("graph instantiate: ") + hipGetErrorString(e)); return nullptr; }
    return exec;
}

bool Engine::graph_for_key(std::map<int, hipGraphExec_t> &cache, int key, int S, bool (Engine::*fn)(int, hipStream_t)) {
    if (cache.count(key)) return true;
    hipGraphExec_t exec = capture(stream_, [&] { return (this->*fn)(S, stream_); });
    if (exec) cache[key] = exec;
    return exec != nullptr;
}

bool Engine::set_slot_state(int S, const std::vector<int> &pos, const std::vector<int> &frame) {
    Q3T_HIP(hipMemcpyAsync(pos_, pos.data(), S * 4, hipMemcpyHostToDevice, stream_));
    Q3T_HIP(hipMemcpyAsync(frame_, frame.data(), S * 4, hipMemcpyHostToDevice, stream_));
    return true;
}

// ------------------------------------------------------------------------------------------ causal prefill
// build_prefill_forward_graph (src/tts_transformer.cpp:1233-1374): the plen prompt rows of n_utt utterances in ONE
// pass of the talker stack -- every projection over all n_utt * plen rows (one weight stream for the whole prompt
// instead of plen), causal attention per utterance (prefill_attn) writing the K/V rows [0, plen) of slot pf_slot_[u]
// directly.  The projections run the kernels of an S_main-slot decode step with its K split (family_b / S_main),
// and the attention reproduces the decode kernel's reduction tree over its first positions, so every row equals the
// S_main-slot step replayed at its position bit for bit (tests/cpp/test_host_api.cpp, tests/test_gpu_prefill.py).
// Outputs: pf_hid_ / pf_logits_ rows u * plen + plen - 1 (final-norm hidden state and codec logits of the last row).
bool Engine::ensure_prefill() {
    if (pf_x_) return true;
    const size_t R = (size_t)max_slots_ * 10, H = c_.hidden, D = c_.head_dim;
    const size_t QKV = (size_t)(c_.n_heads + 2 * c_.n_kv) * D;
    pf_x_ = dalloc<float>(R * H);
    pf_xn_ = dalloc<uint16_t>(R * H);
    pf_parts_ = dalloc<float>(4 * R * H);
    pf_qkv_ = dalloc<float>(R * QKV);
    pf_attn_ = dalloc<uint16_t>(R * c_.n_heads * D);
    pf_hmlp_ = dalloc<uint16_t>(R * c_.inter);
    pf_hid_ = dalloc<float>(R * H);
    pf_logits_ = dalloc<float>(R * c_.codec_vocab);
    pf_slot_ = dalloc<int>(max_slots_);
    pf_off_ = dalloc<int>(max_slots_);
    pf_len_ = dalloc<int>(max_slots_);
    if (!pf_x_ || !pf_xn_ || !pf_parts_ || !pf_qkv_ || !pf_attn_ || !pf_hmlp_ || !pf_hid_ || !pf_logits_ || !pf_slot_ ||
        !pf_off_ || !pf_len_) {
        set_error("device allocation failed");
        return false;
    }
    return true;
}

// the captured body over `rows` rows: plen > 0 the uniform form (rows = n_utt * plen), plen == 0 the ragged one, whose
// attention takes each utterance's first row and row count from pf_off_ / pf_len_ (so one body serves every mix of
// lengths with that total)
bool Engine::enqueue_prefill_rows(int S_main, int n_utt, int plen, int rows, hipStream_t s) {
    const bool mm = use_mm(S_main);
    PrefillAttnParams pf;
    pf.slot = pf_slot_; pf.n_utt = n_utt; pf.plen = plen;
    if (plen == 0) { pf.row_off = pf_off_; pf.row_count = pf_len_; }
    StackRun r;
    r.buf = prefill_bufs(); r.kv = talker_cache();
    r.family = S_main; r.pf = &pf;
    r.final_norm = out_norm_; r.final_side = pf_hid_;
    if (mm ? !decoder_stack_mm(c_, opt_, L_, rows, r, s) : !decoder_stack(c_, L_, rows, r, s)) return false;
    GemvParams h;   // final RMSNorm (hidden side output) + codec head over every row, as the S_main-slot step
    h.W = codec_head_; h.N = c_.codec_vocab; h.nw = out_norm_; h.side_out = pf_hid_; h.out_f32 = pf_logits_;
    h.family_b = S_main; h.force_mm = mm;
    return head_gemv(c_, h, r.buf, mm, rows, s);
}

// src: [n_utt][10][H] prompt rows (rows [0, plen) of each used); pf_slot_[0, n_utt) must hold the target slots
bool Engine::prefill(int n_utt, int plen, const float *src, int S_main, hipStream_t s) {
    const int H = c_.hidden;
    if (n_utt <= 0 || n_utt > max_slots_ || plen < 1 || plen > 10 || S_main < 1 || S_main > 4096) {
        set_error("prefill: bad shape");
        return false;
    }
    if (!ensure_prefill()) return false;
    if (!mm_ok_) S_main = 1;   // every step of this model runs the 1-slot vector kernels (fam1_)
    Q3T_HIP(hipMemcpy2DAsync(pf_x_, (size_t)plen * H * 4, src, (size_t)10 * H * 4, (size_t)plen * H * 4, n_utt,
                             hipMemcpyDeviceToDevice, s));
    const int key = (S_main * 1024 + n_utt) * 16 + plen;
    if (!g_prefill_.count(key)) {
        hipGraphExec_t exec = capture(s, [&] { return enqueue_prefill_rows(S_main, n_utt, plen, n_utt * plen, s); });
        if (!exec) return false;
        g_prefill_[key] = exec;
    }
    Q3T_HIP(hipGraphLaunch(g_prefill_[key], s));
    return true;
}

// src: the packed prompt rows, utterance u's lens[u] rows behind those of u - 1; pf_slot_[0, n_utt) must hold the target
// slots.  The decoder stack's per-row arithmetic does not depend on the other rows, so every row is what the uniform
// form computes for it.  Outputs as there, at the packed row offsets.
bool Engine::prefill_ragged(int n_utt, const int *lens, const float *src, int S_main, hipStream_t s, PromptScratch &ps) {
    const int H = c_.hidden;
    if (n_utt <= 0 || n_utt > max_slots_ || n_utt >= 1024 || S_main < 1 || S_main > 4096) { set_error("prefill: bad shape"); return false; }
    std::vector<int> &rag = ps.rag_host;   // a member: the (pageable) source outlives the copies
    rag.assign((size_t)2 * n_utt, 0);
    int total = 0;
    for (int u = 0; u < n_utt; ++u) {
        if (lens[u] < 1 || lens[u] > 10) { set_error("prefill: rows per utterance must be in [1, 10]"); return false; }
        rag[u] = total;
        rag[n_utt + u] = lens[u];
        total += lens[u];
    }
    if (!ensure_prefill()) return false;
    if (!mm_ok_) S_main = 1;
    Q3T_HIP(hipMemcpyAsync(pf_off_, rag.data(), n_utt * 4, hipMemcpyHostToDevice, s));
    Q3T_HIP(hipMemcpyAsync(pf_len_, rag.data() + n_utt, n_utt * 4, hipMemcpyHostToDevice, s));
    Q3T_HIP(hipMemcpyAsync(pf_x_, src, (size_t)total * H * 4, hipMemcpyDeviceToDevice, s));
    const long long key = ((long long)S_main * 1024 + n_utt) * 16384 + total;
    if (!g_prefill_rag_.count(key)) {
        hipGraphExec_t exec = capture(s, [&] { return enqueue_prefill_rows(S_main, n_utt, 0, total, s); });
        if (!exec) return false;
        g_prefill_rag_[key] = exec;
    }
    Q3T_HIP(hipGraphLaunch(g_prefill_rag_[key], s));
    return true;
}

// ------------------------------------------------------------------------------------------ prefill pieces
bool Engine::alloc_prompt_scratch(PromptScratch &ps, float *spk) {
    const int S = max_slots_, H = c_.hidden;
    ps.cap = S * (max_trailing_ + 16);
    ps.idx = dalloc<int>(ps.cap);
    ps.h = dalloc<uint16_t>((size_t)ps.cap * c_.text_dim);
    ps.out = dalloc<float>((size_t)ps.cap * H);
    ps.recipe = dalloc<RowRecipe>(ps.cap);
    ps.rows = dalloc<float>((size_t)S * 10 * H);
    ps.spk = spk ? spk : dalloc<float>((size_t)S * H);
    if (!ps.idx || !ps.h || !ps.out || !ps.recipe || !ps.rows || !ps.spk) { set_error("device allocation failed"); return false; }
    return true;
}

bool Engine::enqueue_text_projection(int n_rows, hipStream_t s, const PromptScratch &ps) {
    return enqueue_text_projection(n_rows, s, ps.idx, ps.h, ps.out, false);
}

bool Engine::enqueue_text_projection(int n_rows, hipStream_t s, const int *idx, uint16_t *h, float *out, bool as_admission) {
    // text_embd row gather -> fc1 + b -> SiLU -> fc2 + b   (tts_transformer.cpp:1050-1055)
    // as_admission: the smallest admission projects 7 rows (plan_rows), so with the matrix-core GEMM on from <= 7 rows
    // every admission runs it, and its per-row arithmetic does not depend on the rows beside it
    const bool mm = as_admission && gemm_mfma_min_batch() <= 7;
    GemvParams a;
    a.W = fc1_; a.N = c_.text_dim; a.K = c_.text_dim; a.B = n_rows;
    a.pro = PRO_F16; a.x = text_embd_; a.ldx = c_.text_dim; a.x_idx = idx;
    a.bias = fc1_b_; a.act = ACT_SILU; a.out_f16 = h; a.ldo = c_.text_dim;
    a.force_mm = mm;
    if (!gemv(a, s)) return false;
    GemvParams b;
    b.W = fc2_; b.N = c_.hidden; b.K = c_.text_dim; b.B = n_rows;
    b.pro = PRO_F16; b.x = h; b.ldx = c_.text_dim;
    b.bias = fc2_b_; b.out_f32 = out; b.ldo = c_.hidden;
    b.force_mm = mm;
    return gemv(b, s);
}

bool Engine::project_text(int n, const int32_t *toks, float *out) {
    if (n <= 0) return true;
    if (n > main_ps_.cap) { set_error("too many text rows"); return false; }
    DeviceLock lk(false, device_);
    for (int i = 0; i < n; ++i)
        if (toks[i] < 0 || toks[i] >= c_.text_vocab) { set_error("text token out of range"); return false; }
    Q3T_HIP(hipMemcpyAsync(main_ps_.idx, toks, n * 4, hipMemcpyHostToDevice, stream_));
    // a row is what an admission (and a text feed) computes for its id, however many ids share the call
    if (!enqueue_text_projection(n, stream_, main_ps_.idx, main_ps_.h, main_ps_.out, true)) return false;
    Q3T_HIP(hipMemcpyAsync(out, main_ps_.out, (size_t)n * c_.hidden * 4, hipMemcpyDeviceToHost, stream_));
    Q3T_HIP(hipStreamSynchronize(stream_));
    return true;
}

namespace {
struct SlotPlan { int rb, n, plen, tcount; };
}

// Prefill assembly for slots 0..n_utt-1 on device (build_prefill_graph, tts_transformer.cpp:1093-1231).
// Projection rows of slot s start at rb: [tts_bos, tts_eos, tts_pad, tok0, tok1, tok2, tok3, tok4 .. tok(n-6)]
static bool plan_rows(const Config &c, int n_utt, const int32_t *const *tokens, const int *n_tokens, int max_trailing,
                      std::vector<int> &idx, std::vector<SlotPlan> &plan) {
    idx.clear();
    plan.clear();
    for (int s = 0; s < n_utt; ++s) {
        const int n = n_tokens[s];
        if (n < 4) { set_error("Need at least 4 text tokens for generation"); return false; }
        const int tcount = std::max(0, n - 9);
        if (tcount + 1 > max_trailing) { set_error("prompt too long for the trailing-text buffer"); return false; }
        SlotPlan p{(int)idx.size(), n, 0, tcount};
        idx.push_back(c.tts_bos); idx.push_back(c.tts_eos); idx.push_back(c.tts_pad);
        for (int i = 0; i < 4; ++i) idx.push_back(tokens[s][i]);
        for (int i = 0; i < tcount; ++i) idx.push_back(tokens[s][4 + i]);
        plan.push_back(p);
    }
    for (int v : idx)
        if (v < 0 || v >= c.text_vocab) { set_error("text token out of range"); return false; }
    return true;
}

// rows of a prompt: 3 text rows, then one per entry of the codec input [think | nothink, think_bos, (language),
// think_eos, (speaker), pad, bos]
int Engine::prompt_len(int language_id, bool has_spk) {
    return 3 + (language_id < 0 ? 3 : 4) + (has_spk ? 1 : 0) + 2;
}

bool Engine::assemble_prompts(PromptScratch &ps, hipStream_t s, const std::vector<PromptEntry> &in, std::vector<int> &plen_out,
                              std::vector<int> &trailing_len) {
    const int H = c_.hidden, n = (int)in.size();
    for (const PromptEntry &e : in)
        if (e.language_id >= c_.codec_vocab) { set_error("language id out of range"); return false; }
    std::vector<const int32_t *> tk(n);
    std::vector<int> nt(n), &idx = ps.idx_host;
    for (int j = 0; j < n; ++j) { tk[j] = in[j].tokens; nt[j] = in[j].n_tokens; }
    std::vector<SlotPlan> plan;
    if (!plan_rows(c_, n, tk.data(), nt.data(), max_trailing_, idx, plan)) return false;
    if ((int)idx.size() > ps.cap) { set_error("too many text rows"); return false; }
    // ---- text projection for every entry, one batched pass
    Q3T_HIP(hipMemcpyAsync(ps.idx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, s));
    if (!enqueue_text_projection((int)idx.size(), s, ps)) return false;
    // ---- prompt / trailing / pad rows
    std::vector<RowRecipe> &rec = ps.recipe_host;
    plen_out.resize(n);
    rec.clear();
    auto crow = [&](int id) { return RowTerm{codec_embd_ + (size_t)id * H, 1}; };
    trailing_len.resize(n);
    for (int j = 0; j < n; ++j) {
        const SlotPlan &p = plan[j];
        const int k = in[j].slot, language_id = in[j].language_id;
        const int plen = prompt_len(language_id, in[j].speaker != nullptr);
        if (in[j].row < 0 || in[j].row + plen > max_slots_ * 10) { set_error("prompt assembly: row out of range"); return false; }
        float *spk_dev = ps.spk + (size_t)k * H;
        if (in[j].speaker) Q3T_HIP(hipMemcpyAsync(spk_dev, in[j].speaker, H * 4, hipMemcpyHostToDevice, s));
        const float *P = ps.out + (size_t)p.rb * H;
        auto prow = [&](int i) { return RowTerm{P + (size_t)i * H, 0}; };
        auto row = [&](float *dst, RowTerm a, RowTerm b = {nullptr, 0}) { rec.push_back(RowRecipe{dst, {a, b, {nullptr, 0}}}); };
        std::vector<RowTerm> cin;
        if (language_id < 0) cin = {crow(c_.nothink), crow(c_.think_bos), crow(c_.think_eos)};
        else cin = {crow(c_.think), crow(c_.think_bos), crow(language_id), crow(c_.think_eos)};
        if (in[j].speaker) cin.push_back(RowTerm{spk_dev, 0});
        cin.push_back(crow(c_.codec_pad));
        cin.push_back(crow(c_.codec_bos));
        const int ol = (int)cin.size() - 1;
        if (3 + ol + 1 != plen) { set_error("prompt assembly: prefill length mismatch"); return false; }
        float *out = ps.rows + (size_t)in[j].row * H;
        for (int r = 0; r < 3; ++r) row(out + (size_t)r * H, prow(3 + r));
        for (int t = 0; t < ol; ++t) row(out + (size_t)(3 + t) * H, t == ol - 1 ? prow(0) : prow(2), cin[t]);
        row(out + (size_t)(plen - 1) * H, prow(6), cin.back());
        float *tr = trailing_ + (size_t)k * max_trailing_ * H;
        for (int i = 0; i < p.tcount; ++i) row(tr + (size_t)i * H, prow(7 + i));
        row(tr + (size_t)p.tcount * H, prow(1));
        row(tts_pad_ + (size_t)k * H, prow(2));
        trailing_len[j] = p.tcount + 1;
        plen_out[j] = plen;
    }
    if ((int)rec.size() > ps.cap) { set_error("recipe overflow"); return false; }
    Q3T_HIP(hipMemcpyAsync(ps.recipe, rec.data(), rec.size() * sizeof(RowRecipe), hipMemcpyHostToDevice, s));
    return rows_recipe(ps.recipe, (int)rec.size(), H, s);
}

bool Engine::prefill_embd(const int32_t *toks, int n, const float *spk, int language_id, float *prefill, int *prefill_len,
                          float *trailing, int *trailing_len, float *tts_pad) {
    // host entry for the parity tests: run the same device assembly as generate() on slot 0
    DeviceLock lk(false, device_);
    const int H = c_.hidden;
    std::vector<int> tl, pl;
    if (!assemble_prompts(main_ps_, stream_, {PromptEntry{toks, n, spk, 0, 0, language_id}}, pl, tl)) return false;
    const int plen = pl[0];
    Q3T_HIP(hipMemcpyAsync(prefill, main_ps_.rows, (size_t)plen * H * 4, hipMemcpyDeviceToHost, stream_));
    Q3T_HIP(hipMemcpyAsync(trailing, trailing_, (size_t)tl[0] * H * 4, hipMemcpyDeviceToHost, stream_));
    Q3T_HIP(hipMemcpyAsync(tts_pad, tts_pad_, (size_t)H * 4, hipMemcpyDeviceToHost, stream_));
    Q3T_HIP(hipStreamSynchronize(stream_));
    *prefill_len = plen;
    *trailing_len = tl[0];
    return true;
}

// ------------------------------------------------------------------------------------------ hot path
bool Engine::set_seed(uint64_t seed, hipStream_t s) {
    seed_host_ = seed;   // a member: the (pageable) source outlives the copy
    Q3T_HIP(hipMemcpyAsync(seed_dev_, &seed_host_, 8, hipMemcpyHostToDevice, s));
    return true;
}

bool Engine::copy_weights_from(Engine &src) {
    DeviceLock lk(false, device_);
    std::vector<WeightArena *> a = weight_arenas(), b = src.weight_arenas();
    if (a.size() != b.size()) { set_error("copy_weights_from: contexts differ in vocoder presence"); return false; }
    for (size_t i = 0; i < a.size(); ++i) {
        if (a[i]->used != b[i]->used) { set_error("copy_weights_from: weight blobs differ in size"); return false; }
        if (a[i]->used) Q3T_HIP(hipMemcpyPeerAsync(a[i]->base, device_, b[i]->base, src.device_, a[i]->used, stream_));
    }
    Q3T_HIP(hipStreamSynchronize(stream_));
    return build_persist_tables();   // the tables derived from the weights, now that they are in place
}

bool Engine::generate(int n_utt, const int32_t *const *tokens, const int *n_tokens, const float *const *speaker,
                      const GenParams &gp, int32_t *codes, int *n_frames, FrameCb on_frames, void *user, int interval,
                      const UttParams *up) {
    if (n_utt <= 0) return true;
    for (int u = 0; u < n_utt; ++u) n_frames[u] = 0;
    if (n_utt > max_slots_) { set_error("n_utt exceeds max_slots"); return false; }
    // a run that launches a persistent grid holds the device alone (persist_exclusive); the others share it
    DeviceLock lk(persist_exclusive(n_utt), device_);
    StreamState st;
    st.delivered.assign(n_utt, 0);
    st.stop_at.assign(n_utt, -1);
    bool fault = false;
    ScopeExit rec_off([&] { rec_on_ = false; });   // the stage entry points and the call-wide paths read the scalars
    if (generate_once(n_utt, tokens, n_tokens, speaker, gp, up, codes, n_frames, on_frames, user, interval, st, &fault))
        return true;
    if (!fault) return false;
    // a persistent launch gave up on a hand-off: nothing it produced was delivered (every chunk is checked before it
    // is handed out); re-run on the launch-per-op graphs, which are bit-identical, skipping the delivered chunks
    if (!persist_recover()) return false;
    return generate_once(n_utt, tokens, n_tokens, speaker, gp, up, codes, n_frames, on_frames, user, interval, st, &fault);
}

bool Engine::check_gen_args(int n_utt, const int32_t *const *tokens, const int *n_tokens, const float *const *speaker,
                            const GenParams &gp, int *plen) {
    if (gp.language_id >= c_.codec_vocab) { set_error("language id out of range"); return false; }
    const bool has_spk = speaker && speaker[0];
    for (int u = 0; u < n_utt; ++u)
        if ((speaker && speaker[u]) != has_spk) { set_error("speaker embedding must be given for all or none of the utterances"); return false; }
    std::vector<int> idx;   // every prompt is validated before anything runs
    std::vector<SlotPlan> plan;
    if (!plan_rows(c_, n_utt, tokens, n_tokens, max_trailing_, idx, plan)) return false;
    *plen = prompt_len(gp.language_id, has_spk);
    if (*plen + gp.max_len + 8 > max_ctx_) { set_error("max_len exceeds the context reserved at ctx creation"); return false; }
    return true;
}

bool Engine::check_utt_args(int n_utt, const int32_t *const *tokens, const int *n_tokens, const float *const *speaker,
                            const GenParams &gp, const UttParams *up, std::vector<UttParams> &ups, std::vector<int> &plen,
                            int id0) {
    ups.assign(up, up + n_utt);
    plen.assign(n_utt, 0);
    for (int u = 0; u < n_utt; ++u) {
        UttParams &r = ups[u];
        const std::string who = "utterance " + std::to_string(id0 + u) + ": ";
        if (r.max_len <= 0) r.max_len = gp.max_len;
        if (r.language_id >= c_.codec_vocab) { set_error(who + "language id out of range"); return false; }
        if (r.max_len > gp.max_len) { set_error(who + "max_len exceeds the call's max_len"); return false; }
        plen[u] = prompt_len(r.language_id, speaker && speaker[u]);
        if (plen[u] + r.max_len + 8 > max_ctx_) { set_error(who + "max_len exceeds the context reserved at ctx creation"); return false; }
        if (r.top_k < 0) { set_error(who + "top_k must be >= 0"); return false; }
        if (!(r.rep_penalty > 0.0f) || !std::isfinite(r.rep_penalty)) { set_error(who + "repetition_penalty must be finite and > 0"); return false; }
        if (!std::isfinite(r.temperature)) { set_error(who + "temperature must be finite"); return false; }
    }
    std::vector<int> idx;
    std::vector<SlotPlan> plan;
    return plan_rows(c_, n_utt, tokens, n_tokens, max_trailing_, idx, plan);
}

bool Engine::resolve_utt_params(int n_utt, const int32_t *const *tokens, const int *n_tokens, const float *const *speaker,
                                const GenParams &gp, const UttParams *up, std::vector<UttParams> &ups, std::vector<int> &plen) {
    if (up) return check_utt_args(n_utt, tokens, n_tokens, speaker, gp, up, ups, plen);
    int plen0 = 0;
    if (!check_gen_args(n_utt, tokens, n_tokens, speaker, gp, &plen0)) return false;
    ups.assign(n_utt, UttParams{gp.language_id, gp.max_len, gp.rep_penalty, gp.temperature, gp.top_k, gp.force_frames});
    plen.assign(n_utt, plen0);
    return true;
}

std::string Engine::check_arrival(int32_t id, const Arrival &a, const GenParams &gp, UttParams *up, int *plen) {
    const std::string who = "utterance " + std::to_string(id) + ": ";
    if (a.n_tokens < 0 || !a.tokens) return who + "no prompt";
    std::vector<UttParams> ups;
    std::vector<int> pl;
    const int32_t *tok = a.tokens;
    const int n_tok = a.n_tokens;
    const float *spk = a.speaker;
    if (!check_utt_args(1, &tok, &n_tok, &spk, gp, &a.up, ups, pl, id)) {
        const std::string &m = last_error();   // (the prompt checks do not name the utterance)
        return m.compare(0, 10, "utterance ") == 0 ? m : who + m;
    }
    *up = ups[0];
    *plen = pl[0];
    return std::string();
}

void Engine::set_gen_params(const GenParams &gp) {
    if (!(gp.temperature == gp_.temperature && gp.top_k == gp_.top_k && gp.rep_penalty == gp_.rep_penalty)) {
        // (the graphs captured with the record pointer bake none of the three: they stay)
        for (auto it = g_frame_.begin(); it != g_frame_.end();) {
            if (it->first & (1 << 30)) { ++it; continue; }
            hipGraphExecDestroy(it->second);
            it = g_frame_.erase(it);
        }
    }
    gp_ = gp;
}

// streaming (frame callback) of generate(): chunk [start, start+interval) of every slot is copied to pinned memory
// behind the frame that completes it and delivered one chunk late, so the GPU keeps running the queued frames
// meanwhile.  The pinned chunks are the context's (chunk_pool_), reused across calls.
class Engine::ChunkStreamer {
public:
    // max_len: the stride of the caller's codes; cap[s]: slot s's own max_len
    ChunkStreamer(Engine &e, int S, int max_len, std::vector<int> cap, FrameCb cb, void *user, int interval, StreamState &st,
                  bool *fault)
        : e_(e), S_(S), max_len_(max_len), cap_(std::move(cap)), interval_(interval), cb_(cb), user_(user), st_(st),
          fault_(fault), n_live_(S) {}
    bool active() const { return cb_ && interval_ > 0; }
    // utterances the callback has not stopped (a fallback re-run regenerates utterances stopped earlier too: their
    // frames are returned)
    int n_live() const { return n_live_; }
    // frame f was launched: if it completes a chunk, queue the chunk's copy behind it and deliver the chunk before
    bool after_frame(int f) {
        if (!active() || (f + 1) % interval_ != 0) return true;
        Chunk c;
        if (!pool_.empty()) { c = pool_.back(); pool_.pop_back(); }
        else if (!take_chunk(c)) return false;
        c.start = f + 1 - interval_;
        for (int s = 0; s < S_; ++s)
            Q3T_HIP(hipMemcpyAsync(c.codes + (size_t)s * interval_ * NCB, e_.codes_ + ((size_t)s * e_.codes_max_len_ + c.start) * NCB,
                                   (size_t)interval_ * NCB * 4, hipMemcpyDeviceToHost, e_.stream_));
        Q3T_HIP(hipMemcpyAsync(c.done, e_.done_, S_ * 4, hipMemcpyDeviceToHost, e_.stream_));
        Q3T_HIP(hipEventRecord(c.ev, e_.stream_));
        pend_.push_back(c);
        if (pend_.size() == 1) return true;
        Chunk front = pend_.front();
        pend_.erase(pend_.begin());
        pool_.push_back(front);
        if (deliver(front)) return true;
        hipStreamSynchronize(e_.stream_);
        return false;
    }
    // after the last frame (codes: the caller's [S][max_len][16], n_frames: each utterance's length): the chunks still
    // pending, then the remainder of every utterance (tts_transformer.cpp:2563-2570)
    bool flush(const int32_t *codes, int *n_frames) {
        if (!active()) return true;
        for (Chunk &c : pend_)
            if (!deliver(c)) return false;
        for (int s = 0; s < S_; ++s) {
            if (st_.stop_at[s] >= 0) { n_frames[s] = std::min(n_frames[s], st_.stop_at[s]); continue; }
            if (n_frames[s] > st_.delivered[s])
                cb_(user_, s, codes + ((size_t)s * max_len_ + st_.delivered[s]) * NCB, n_frames[s] - st_.delivered[s], NCB);
        }
        return true;
    }

private:
    static constexpr int NCB = 16;
    struct Chunk { int start; int32_t *codes; int *done; hipEvent_t ev; };
    bool take_chunk(Chunk &c) {   // the next pinned chunk of the context's pool, grown to this call's chunk size
        PinnedChunk *pc = nullptr;
        if (!e_.pinned_chunk(next_chunk_++, ((size_t)S_ * interval_ * NCB + S_) * 4, &pc)) return false;
        c.codes = pc->codes;
        c.done = pc->codes + (size_t)S_ * interval_ * NCB;
        c.ev = pc->ev;
        return true;
    }
    // a chunk is handed to the caller only once the persistent kernels behind it are known to be fault-free
    bool deliver(Chunk &c) {
        Q3T_HIP(hipEventSynchronize(c.ev));
        if (e_.persist_error()) { *fault_ = true; return false; }
        for (int s = 0; s < S_; ++s) {
            if (st_.stop_at[s] >= 0) continue;
            const int nf = frames_of(c.done[s], cap_[s]);
            if (nf < c.start + interval_) continue;   // partial chunks go to the final flush, as in the reference
            if (c.start + interval_ <= st_.delivered[s]) continue;   // delivered before a fallback re-run
            st_.delivered[s] = c.start + interval_;
            if (!cb_(user_, s, c.codes + (size_t)s * interval_ * NCB, interval_, NCB)) {
                const int d = st_.stop_at[s] = c.start + interval_;
                Q3T_HIP(hipMemcpyAsync(e_.done_ + s, &d, 4, hipMemcpyHostToDevice, e_.stream_));
                Q3T_HIP(hipStreamSynchronize(e_.stream_));   // &d is a stack value
                --n_live_;
            }
        }
        return true;
    }
    Engine &e_;
    const int S_, max_len_;
    const std::vector<int> cap_;
    const int interval_;
    const FrameCb cb_;
    void *const user_;
    StreamState &st_;
    bool *const fault_;
    int n_live_;
    size_t next_chunk_ = 0;           // chunk_pool_[0, next_chunk_) are in use by this call
    std::vector<Chunk> pend_, pool_;  // copies in flight, oldest first; chunks delivered and free for reuse
};

bool Engine::generate_once(int n_utt, const int32_t *const *tokens, const int *n_tokens, const float *const *speaker,
                           const GenParams &gp, const UttParams *up, int32_t *codes, int *n_frames, FrameCb on_frames,
                           void *user, int interval, StreamState &st, bool *fault) {
    *fault = false;
    const int S = n_utt, H = c_.hidden, NCB = 16;
    for (int s = 0; s < S; ++s) n_frames[s] = 0;
    if (gp.max_len <= 0) return true;
    // the call-wide form: one record for every slot, one prompt length, the uniform prefill.  With records (up): each
    // slot's own, the prompt rows packed and the ragged prefill
    std::vector<UttParams> ups;
    std::vector<int> posv;
    if (!resolve_utt_params(S, tokens, n_tokens, speaker, gp, up, ups, posv)) return false;
    const int plen = posv[0];   // (the call-wide form's)
    int loop_len = 0;           // the longest record: a slot past its own max_len runs on, its frames are not returned
    for (int s = 0; s < S; ++s) loop_len = std::max(loop_len, ups[s].max_len);
    rec_on_ = up && S > 1;
    if (!up) set_gen_params(gp);
    else if (S == 1) {   // one slot: its utterance's values into the scalars the one-slot kernels read
        GenParams g1 = gp;
        g1.temperature = ups[0].temperature; g1.top_k = ups[0].top_k; g1.rep_penalty = ups[0].rep_penalty;
        set_gen_params(g1);
    }
    if (!set_seed(gp.seed, stream_)) return false;
    if (!ensure_prefill()) return false;
    Event e0, e1, e2;
    Q3T_HIP(hipEventRecord(e0, stream_));
    // ---- prompt, trailing and pad rows of every slot
    std::vector<PromptEntry> in(S);
    for (int s = 0, row = 0; s < S; row += posv[s], ++s)
        in[s] = PromptEntry{tokens[s], n_tokens[s], speaker ? speaker[s] : nullptr, s, up ? row : s * 10, ups[s].language_id};
    std::vector<int> tl, pl, ntok(n_tokens, n_tokens + S), force(S), frame0(S, 0), done0(S, -1);
    for (int s = 0; s < S; ++s) force[s] = ups[s].force_frames;
    if (!assemble_prompts(main_ps_, stream_, in, pl, tl)) return false;
    if (pl != posv) { set_error("generate: prefill length mismatch"); return false; }
    if (rec_on_) {
        std::vector<SelRec> &recs = main_ps_.rec_host;   // a member: the (pageable) source outlives the copy
        recs.resize(S);
        for (int s = 0; s < S; ++s) recs[s] = sel_rec(ups[s]);
        Q3T_HIP(hipMemcpyAsync(sel_rec_, recs.data(), S * sizeof(SelRec), hipMemcpyHostToDevice, stream_));
    }
    Q3T_HIP(hipMemcpyAsync(trailing_len_, tl.data(), S * 4, hipMemcpyHostToDevice, stream_));
    Q3T_HIP(hipMemcpyAsync(n_tokens_, ntok.data(), S * 4, hipMemcpyHostToDevice, stream_));
    Q3T_HIP(hipMemcpyAsync(force_, force.data(), S * 4, hipMemcpyHostToDevice, stream_));
    Q3T_HIP(hipMemcpyAsync(done_, done0.data(), S * 4, hipMemcpyHostToDevice, stream_));
    Q3T_HIP(hipMemsetAsync(seen_, 0, (size_t)S * c_.codec_vocab, stream_));
    Q3T_HIP(hipMemsetAsync(codes_, 0, (size_t)S * codes_max_len_ * NCB * 4, stream_));
    // ---- prefill: one causal pass over the plen rows of every slot; the last row's hidden state / logits per slot
    Q3T_HIP(hipMemcpyAsync(pf_slot_, slot_iota_, S * 4, hipMemcpyDeviceToDevice, stream_));
    const int S_main = policy_slots_ > 0 ? policy_slots_ : S;
    if (up) {
        if (!prefill_ragged(S, posv.data(), main_ps_.rows, S_main, stream_, main_ps_)) return false;
        const size_t V = c_.codec_vocab;
        for (int s = 0; s < S; ++s) {   // each slot's last row, by its packed offset
            const size_t r = (size_t)in[s].row + posv[s] - 1;
            Q3T_HIP(hipMemcpyAsync(hidden_ + (size_t)s * H, pf_hid_ + r * H, H * 4, hipMemcpyDeviceToDevice, stream_));
            Q3T_HIP(hipMemcpyAsync(logits_ + s * V, pf_logits_ + r * V, V * 4, hipMemcpyDeviceToDevice, stream_));
        }
    } else {
        if (!prefill(S, plen, main_ps_.rows, S_main, stream_)) return false;
        Q3T_HIP(hipMemcpy2DAsync(hidden_, H * 4, pf_hid_ + (size_t)(plen - 1) * H, (size_t)plen * H * 4, H * 4, S,
                                 hipMemcpyDeviceToDevice, stream_));
        Q3T_HIP(hipMemcpy2DAsync(logits_, (size_t)c_.codec_vocab * 4, pf_logits_ + (size_t)(plen - 1) * c_.codec_vocab,
                                 (size_t)plen * c_.codec_vocab * 4, (size_t)c_.codec_vocab * 4, S, hipMemcpyDeviceToDevice, stream_));
    }
    if (!set_slot_state(S, posv, frame0)) return false;
    if (fused_select_ && !select_tokens(select_spec(SEL_CB0, gp_, 0, 0), logits_, S, stream_)) return false;
#ifdef Q3T_DEV
    const bool dbg = std::getenv("Q3T_DEBUG") != nullptr;
#else
    constexpr bool dbg = false;
#endif
    if (dbg) { fprintf(stderr, "[q3t] prefill enqueued (plen %d)\n", plen); fflush(stderr); }
    Q3T_HIP(hipEventRecord(e1, stream_));
    // ---- frame loop: one graph per frame; done flags polled every 16 frames
    const int fkey = frame_key(S);
    if (!graph_for_key(g_frame_, fkey, S, &Engine::enqueue_frame)) return false;
    if (!ensure_pinned((size_t)S * 4)) return false;
    int *done_h = static_cast<int *>(pin_);
    std::vector<int> cap(S);
    for (int s = 0; s < S; ++s) cap[s] = ups[s].max_len;
    ChunkStreamer streamer(*this, S, gp.max_len, cap, on_frames, user, interval, st, fault);
    bool all_done = false;
    for (int f = 0; f < loop_len && !all_done && streamer.n_live() > 0; ++f) {
        if (!persist_fault_hook(S, (persist_ ? 1 : 0) + (persist_cp_ ? 1 : 0))) return false;
        Q3T_HIP(hipGraphLaunch(g_frame_[fkey], stream_));
        if (dbg) { fprintf(stderr, "[q3t] frame %d launched\n", f); fflush(stderr); }
        if (!streamer.after_frame(f)) return false;
        if ((f + 1) % poll_every_ == 0 && f + 1 < loop_len) {
            Q3T_HIP(hipMemcpyAsync(done_h, done_, S * 4, hipMemcpyDeviceToHost, stream_));
            Q3T_HIP(hipStreamSynchronize(stream_));
            all_done = true;
            for (int s = 0; s < S; ++s) all_done = all_done && (done_h[s] >= 0 || f + 1 >= cap[s]);
        }
    }
    Q3T_HIP(hipEventRecord(e2, stream_));
    if (dbg) { fprintf(stderr, "[q3t] frame loop enqueued\n"); fflush(stderr); }
    Q3T_HIP(hipMemcpyAsync(done_h, done_, S * 4, hipMemcpyDeviceToHost, stream_));
    // one 1-D copy per slot into the caller's [n_utt][max_len][16] buffer (a pitched 2-D copy into pageable host memory
    // was observed to overrun the destination under rocprofv3 on ROCm 7.2)
    // (a slot's rows up to its own max_len: the rest of its stride stays as the caller passed it)
    for (int s = 0; s < S; ++s)
        Q3T_HIP(hipMemcpyAsync(codes + (size_t)s * gp.max_len * NCB, codes_ + (size_t)s * codes_max_len_ * NCB,
                               (size_t)cap[s] * NCB * 4, hipMemcpyDeviceToHost, stream_));
    Q3T_HIP(hipStreamSynchronize(stream_));
    if (dbg) { fprintf(stderr, "[q3t] frame loop done\n"); fflush(stderr); }
    if (persist_error()) {
        set_error("persistent kernel: an in-launch hand-off timed out");
        *fault = true;
        return false;
    }
    for (int s = 0; s < S; ++s) n_frames[s] = frames_of(done_h[s], cap[s]);
    if (!streamer.flush(codes, n_frames)) return false;
    float ms1 = 0, ms2 = 0;
    hipEventElapsedTime(&ms1, e0, e1);
    hipEventElapsedTime(&ms2, e1, e2);
    last_prefill_ms = ms1;
    last_frames_ms = ms2;
    return true;
}

bool Engine::time_stage(int stage, int S, int pos, int iters, double *ms) {
    if (S <= 0 || S > max_slots_ || pos < 0 || pos >= max_ctx_ || iters <= 0) { set_error("time_stage: bad arguments"); return false; }
    DeviceLock lk(persist_exclusive(S), device_);
    std::vector<int> pv(S, pos), fr(S, 0), dn(S, -1);
    Q3T_HIP(hipMemcpyAsync(pos_, pv.data(), S * 4, hipMemcpyHostToDevice, stream_));
    Q3T_HIP(hipMemcpyAsync(frame_, fr.data(), S * 4, hipMemcpyHostToDevice, stream_));
    Q3T_HIP(hipMemcpyAsync(done_, dn.data(), S * 4, hipMemcpyHostToDevice, stream_));
    hipGraphExec_t g = nullptr;
    if (stage == 0) { if (!graph_for(g_talker_, S, &Engine::enqueue_talker_step)) return false; g = g_talker_[S]; }
    else { if (!graph_for(g_cp_, S, &Engine::enqueue_cp_only)) return false; g = g_cp_[S]; }
    Q3T_HIP(hipGraphLaunch(g, stream_));   // warm
    // one event pair around EACH replay, on the stream the kernels run on: the mean is the replay's own duration (for
    // the persistent stages, the one kernel's), without the host-side gap between two graph launches
    std::vector<Event> ev(2 * (size_t)iters);
    for (int i = 0; i < iters; ++i) {
        Q3T_HIP(hipEventRecord(ev[2 * i], stream_));
        Q3T_HIP(hipGraphLaunch(g, stream_));
        Q3T_HIP(hipEventRecord(ev[2 * i + 1], stream_));
    }
    Q3T_HIP(hipEventSynchronize(ev.back()));
    double sum = 0.0;
    for (int i = 0; i < iters; ++i) {
        float t = 0;
        hipEventElapsedTime(&t, ev[2 * i], ev[2 * i + 1]);
        sum += t;
    }
    *ms = sum / iters;
    if (persist_error()) {   // time the launch-per-op fallback instead of a faulted persistent launch
        if (!persist_recover()) return false;
        return time_stage(stage, S, pos, iters, ms);
    }
    return true;
}

// ------------------------------------------------------------------------------------------ test entry points
bool Engine::talker_prefill(int n_utt, int n_rows, const float *embd, int family_slots, float *hidden, float *logits) {
    if (n_utt <= 0 || n_utt > max_slots_) { set_error("bad utterance count"); return false; }
    if (n_rows <= 0 || n_rows > 10 || n_rows > max_ctx_) { set_error("prefill rows must be in [1, 10]"); return false; }
    if (family_slots < 0 || family_slots > 4096) { set_error("bad family slot count"); return false; }
    const int H = c_.hidden, V = c_.codec_vocab;
    DeviceLock lk(false, device_);
    if (!ensure_prefill()) return false;
    Q3T_HIP(hipMemcpy2DAsync(main_ps_.rows, (size_t)10 * H * 4, embd, (size_t)n_rows * H * 4, (size_t)n_rows * H * 4, n_utt,
                             hipMemcpyHostToDevice, stream_));
    Q3T_HIP(hipMemcpyAsync(pf_slot_, slot_iota_, n_utt * 4, hipMemcpyDeviceToDevice, stream_));
    if (!prefill(n_utt, n_rows, main_ps_.rows, family_slots > 0 ? family_slots : n_utt, stream_)) return false;
    if (hidden) Q3T_HIP(hipMemcpyAsync(hidden, pf_hid_, (size_t)n_utt * n_rows * H * 4, hipMemcpyDeviceToHost, stream_));
    if (logits)
        Q3T_HIP(hipMemcpy2DAsync(logits, (size_t)V * 4, pf_logits_ + (size_t)(n_rows - 1) * V, (size_t)n_rows * V * 4,
                                 (size_t)V * 4, n_utt, hipMemcpyDeviceToHost, stream_));
    Q3T_HIP(hipStreamSynchronize(stream_));
    return true;
}

bool Engine::talker_prefill_ragged(int n_utt, const int *n_rows, const float *embd, int family_slots, float *hidden,
                                   float *logits) {
    if (n_utt <= 0 || n_utt > max_slots_) { set_error("bad utterance count"); return false; }
    if (family_slots < 0 || family_slots > 4096) { set_error("bad family slot count"); return false; }
    int total = 0;
    for (int u = 0; u < n_utt; ++u) {
        if (n_rows[u] <= 0 || n_rows[u] > 10 || n_rows[u] > max_ctx_) { set_error("prefill rows must be in [1, 10]"); return false; }
        total += n_rows[u];
    }
    const int H = c_.hidden, V = c_.codec_vocab;
    DeviceLock lk(false, device_);
    if (!ensure_prefill()) return false;
    Q3T_HIP(hipMemcpyAsync(main_ps_.rows, embd, (size_t)total * H * 4, hipMemcpyHostToDevice, stream_));
    Q3T_HIP(hipMemcpyAsync(pf_slot_, slot_iota_, n_utt * 4, hipMemcpyDeviceToDevice, stream_));
    if (!prefill_ragged(n_utt, n_rows, main_ps_.rows, family_slots > 0 ? family_slots : n_utt, stream_, main_ps_)) return false;
    if (hidden) Q3T_HIP(hipMemcpyAsync(hidden, pf_hid_, (size_t)total * H * 4, hipMemcpyDeviceToHost, stream_));
    if (logits)
        for (int u = 0, row = 0; u < n_utt; row += n_rows[u], ++u)   // each utterance's last row
            Q3T_HIP(hipMemcpyAsync(logits + (size_t)u * V, pf_logits_ + (size_t)(row + n_rows[u] - 1) * V, (size_t)V * 4,
                                   hipMemcpyDeviceToHost, stream_));
    Q3T_HIP(hipStreamSynchronize(stream_));
    return true;
}

bool Engine::talker_forward(int S, const float *embd, const int *pos, float *hidden, float *logits) {
    if (S <= 0 || S > max_slots_) { set_error("bad slot count"); return false; }
    for (int s = 0; s < S; ++s) if (pos[s] < 0 || pos[s] >= max_ctx_) { set_error("Context length exceeded"); return false; }
    const int H = c_.hidden;
    DeviceLock lk(persist_exclusive(S), device_);
    for (int attempt = 0; attempt < 2; ++attempt) {
        Q3T_HIP(hipMemcpyAsync(x_, embd, (size_t)S * H * 4, hipMemcpyHostToDevice, stream_));
        Q3T_HIP(hipMemcpyAsync(pos_, pos, S * 4, hipMemcpyHostToDevice, stream_));
        if (!graph_for(g_talker_, S, &Engine::enqueue_talker_step)) return false;
        Q3T_HIP(hipGraphLaunch(g_talker_[S], stream_));
        if (hidden) Q3T_HIP(hipMemcpyAsync(hidden, hidden_, (size_t)S * H * 4, hipMemcpyDeviceToHost, stream_));
        if (logits) Q3T_HIP(hipMemcpyAsync(logits, logits_, (size_t)S * c_.codec_vocab * 4, hipMemcpyDeviceToHost, stream_));
        Q3T_HIP(hipStreamSynchronize(stream_));
        if (!persist_error()) return true;
        if (!persist_recover()) return false;   // re-run this position on the launch-per-op graph
    }
    set_error("talker step: persistent fallback failed");
    return false;
}

bool Engine::codepred_frame(int S, const float *hidden, const int *cb0, float temperature, int top_k, uint64_t seed,
                            int frame, int32_t *codes15, float *logits_all) {
    if (S <= 0 || S > max_slots_) { set_error("bad slot count"); return false; }
    const int H = c_.hidden;
    for (int s = 0; s < S; ++s) if (cb0[s] < 0 || cb0[s] >= c_.codec_vocab) { set_error("cb0 out of range"); return false; }
    DeviceLock lk(persist_exclusive(S), device_);
    GenParams gp = gp_;
    gp.temperature = temperature; gp.top_k = top_k; gp.seed = seed;
    set_gen_params(gp);
    if (!set_seed(seed, stream_)) return false;
    Q3T_HIP(hipMemcpyAsync(hidden_, hidden, (size_t)S * H * 4, hipMemcpyHostToDevice, stream_));
    std::vector<int> tk0((size_t)S * 16, 0);
    for (int s = 0; s < S; ++s) tk0[(size_t)s * 16] = cb0[s];
    Q3T_HIP(hipMemcpyAsync(tokens_, tk0.data(), tk0.size() * 4, hipMemcpyHostToDevice, stream_));
    std::vector<int> fr(S, frame), dn(S, -1);
    Q3T_HIP(hipMemcpyAsync(frame_, fr.data(), S * 4, hipMemcpyHostToDevice, stream_));
    Q3T_HIP(hipMemcpyAsync(done_, dn.data(), S * 4, hipMemcpyHostToDevice, stream_));
    if (!enqueue_cp_frame(S, stream_, logits_all)) return false;
    std::vector<int> tk((size_t)S * 16);
    Q3T_HIP(hipMemcpyAsync(tk.data(), tokens_, tk.size() * 4, hipMemcpyDeviceToHost, stream_));
    Q3T_HIP(hipStreamSynchronize(stream_));
    if (persist_error()) {   // re-run the frame on the per-op launches
        if (!persist_recover()) return false;
        Q3T_HIP(hipMemcpyAsync(tokens_, tk0.data(), tk0.size() * 4, hipMemcpyHostToDevice, stream_));
        if (!enqueue_cp_frame(S, stream_, logits_all)) return false;
        Q3T_HIP(hipMemcpyAsync(tk.data(), tokens_, tk.size() * 4, hipMemcpyDeviceToHost, stream_));
        Q3T_HIP(hipStreamSynchronize(stream_));
    }
    for (int s = 0; s < S; ++s) for (int i = 0; i < 15; ++i) codes15[s * 15 + i] = tk[(size_t)s * 16 + 1 + i];
    return true;
}

bool Engine::cb0_select_host(int S, const float *logits, const uint8_t *seen, const int *frame, const int *n_tokens,
                             const GenParams &gp, int *tok) {
    if (S <= 0 || S > max_slots_) { set_error("bad slot count"); return false; }
    const int V = c_.codec_vocab;
    DeviceLock lk(false, device_);
    Q3T_HIP(hipMemcpyAsync(logits_, logits, (size_t)S * V * 4, hipMemcpyHostToDevice, stream_));
    Q3T_HIP(hipMemcpyAsync(seen_, seen, (size_t)S * V, hipMemcpyHostToDevice, stream_));
    Q3T_HIP(hipMemcpyAsync(frame_, frame, S * 4, hipMemcpyHostToDevice, stream_));
    Q3T_HIP(hipMemcpyAsync(n_tokens_, n_tokens, S * 4, hipMemcpyHostToDevice, stream_));
    std::vector<int> force(S, gp.force_frames), dn(S, -1);
    Q3T_HIP(hipMemcpyAsync(force_, force.data(), S * 4, hipMemcpyHostToDevice, stream_));
    Q3T_HIP(hipMemcpyAsync(done_, dn.data(), S * 4, hipMemcpyHostToDevice, stream_));
    SelectSpec sp = select_spec(SEL_CB0, gp, 0, 0);
    sp.seed_dev = nullptr;
    if (!select_tokens(sp, logits_, S, stream_)) return false;
    std::vector<int> tk((size_t)S * 16);
    Q3T_HIP(hipMemcpyAsync(tk.data(), tokens_, tk.size() * 4, hipMemcpyDeviceToHost, stream_));
    Q3T_HIP(hipStreamSynchronize(stream_));
    for (int s = 0; s < S; ++s) tok[s] = tk[(size_t)s * 16];
    return true;
}

}  // namespace q3t
