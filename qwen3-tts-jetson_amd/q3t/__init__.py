"""Python host mirror of the MI355X Qwen3-TTS decode path (ctypes over include/q3t_backend.h / libq3t.so).

The compute runs in libq3t.so (hand-written gfx950 HIP kernels).  There is NO CPU fallback: importing this
module fails loudly if the in-tree extension is missing, and every call raises Q3TError with
q3t_last_error() when the C ABI reports failure (the reference's bool + get_error() convention).
"""
import collections
import ctypes as C
import os
import threading
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# Q3T_DEV_LIB=1 loads the development build (make -C csrc DEV=1: debug hooks for tools/dev), Q3T_DEV_LIB=<name> an
# experiment build (make -C csrc VARIANT=<name>: libq3t_<name>.so); never the default
_dev = os.environ.get("Q3T_DEV_LIB", "")
LIB_PATH = os.path.join(_HERE, "libq3t.so" if not _dev else "libq3t_dev.so" if _dev == "1" else f"libq3t_{_dev}.so")

VOCODER_FULL = 0
VOCODER_CHUNK40 = 1


class Q3TError(RuntimeError):
    pass


if not os.path.exists(LIB_PATH):
    raise ImportError(f"libq3t.so not built at {LIB_PATH}: run `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(make -C qwen3-tts-jetson_amd/csrc)")

_lib = C.CDLL(LIB_PATH)


class Config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "hidden", "n_layers", "n_heads", "n_kv_heads", "head_dim", "intermediate", "codec_vocab", "n_codebooks",
        "text_vocab", "text_dim", "cp_layers", "cp_vocab", "codec_eos", "has_vocoder", "sample_rate", "max_slots",
        "max_ctx", "cp_hidden", "cp_intermediate", "cp_heads", "cp_kv_heads", "has_mtp")]


class GenParams(C.Structure):
    _fields_ = [("max_len", C.c_int32), ("language_id", C.c_int32), ("repetition_penalty", C.c_float),
                ("temperature", C.c_float), ("top_k", C.c_int32), ("seed", C.c_uint64), ("force_frames", C.c_int32)]


class UttParams(C.Structure):
    """q3t_utt_params: one utterance's own language, max_len and sampling values"""
    _fields_ = [("language_id", C.c_int32), ("max_len", C.c_int32), ("repetition_penalty", C.c_float),
                ("temperature", C.c_float), ("top_k", C.c_int32), ("force_frames", C.c_int32)]


_P, _I, _F = C.c_void_p, C.c_int, C.c_float
_fp = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
_ip = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_lib.q3t_last_error.restype = C.c_char_p
_lib.q3t_default_params.argtypes = [C.POINTER(GenParams)]
_lib.q3t_ctx_create.argtypes = [C.c_char_p, C.c_char_p, _I, _I, _I, C.POINTER(_P)]
_lib.q3t_ctx_destroy.argtypes = [_P]
_lib.q3t_get_config.argtypes = [_P, C.POINTER(Config)]
_lib.q3t_generate.argtypes = [_P, _I, C.POINTER(C.POINTER(C.c_int32)), _ip, C.POINTER(C.POINTER(C.c_float)),
                              C.POINTER(GenParams), _ip, _ip]
_lib.q3t_generate_queue.argtypes = [_P, _I, C.POINTER(C.POINTER(C.c_int32)), _ip, C.POINTER(C.POINTER(C.c_float)),
                                    C.POINTER(GenParams), _ip, _ip, C.c_int32]
FRAME_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32)
_lib.q3t_generate_stream.argtypes = [_P, _I, C.POINTER(C.POINTER(C.c_int32)), _ip, C.POINTER(C.POINTER(C.c_float)),
                                     C.POINTER(GenParams), _ip, _ip, FRAME_CB, C.c_void_p, C.c_int32]
QUEUE_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.POINTER(C.c_int32)),
                       C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32))
_lib.q3t_generate_queue_stream.argtypes = [_P, _I, C.POINTER(C.POINTER(C.c_int32)), _ip, C.POINTER(C.POINTER(C.c_float)),
                                           C.POINTER(GenParams), _P, _ip, C.c_int32, QUEUE_CB, C.c_void_p, C.c_int32]
_lib.q3t_utt_params_from.argtypes = [C.POINTER(GenParams), C.POINTER(UttParams)]
_lib.q3t_utt_params_from.restype = None
_lib.q3t_generate_utt.argtypes = [_P, _I, C.POINTER(C.POINTER(C.c_int32)), _ip, C.POINTER(C.POINTER(C.c_float)),
                                  C.POINTER(GenParams), C.POINTER(UttParams), _ip, _ip, _P, C.c_void_p, C.c_int32]
_lib.q3t_generate_queue_utt.argtypes = [_P, _I, C.POINTER(C.POINTER(C.c_int32)), _ip, C.POINTER(C.POINTER(C.c_float)),
                                        C.POINTER(GenParams), C.POINTER(UttParams), _P, _ip, C.c_int32, _P, C.c_void_p,
                                        C.c_int32]
TEXT_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.POINTER(C.c_int32)),
                      C.POINTER(C.c_int32), C.POINTER(C.c_int32))
_lib.q3t_generate_queue_text.argtypes = [_P, _I, C.POINTER(C.POINTER(C.c_int32)), _ip, C.POINTER(C.POINTER(C.c_float)),
                                         C.POINTER(GenParams), _P, _P, _P, _ip, _P, C.c_int32, _P, C.c_void_p, C.c_int32,
                                         _P, C.c_void_p]
_lib.q3t_text_feed_stats.argtypes = [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                     C.POINTER(C.c_double)]


class Arrival(C.Structure):
    """q3t_arrival: one utterance handed to the open queue"""
    _fields_ = [("tokens", C.POINTER(C.c_int32)), ("n_tokens", C.c_int32), ("speaker", C.POINTER(C.c_float)),
                ("up", UttParams), ("key", C.c_uint64)]


ARRIVE_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Arrival),
                        C.POINTER(C.c_int32), C.POINTER(C.c_int32))
_lib.q3t_generate_queue_open.argtypes = [_P, C.POINTER(GenParams), C.c_int32, C.c_int32, ARRIVE_CB, QUEUE_CB, C.c_void_p,
                                         C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
_lib.q3t_check_utt.argtypes = [_P, _P, C.c_int32, _P, C.POINTER(GenParams), C.POINTER(UttParams)]
_lib.q3t_talker_prefill_ragged.argtypes = [_P, _I, _ip, _fp, _I, _P, _P]
COMM_ID_BYTES = 128
_lib.q3t_comm_unique_id.argtypes = [C.c_char_p]
_lib.q3t_ctx_create_shared.argtypes = [C.c_char_p, C.c_char_p, _I, _I, _I, _I, _I, C.c_char_p, C.POINTER(_P)]
_lib.q3t_ctx_create_replica.argtypes = [_P, _I, _I, _I, C.POINTER(_P)]
_lib.q3t_plan_weight_layout.argtypes = [C.c_char_p, _P, _I, C.POINTER(_I), C.POINTER(C.c_uint64)]
_lib.q3t_comm_allreduce_max.argtypes = [_P, np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS"), _I]
_lib.q3t_set_mfma_min_batch.argtypes = [_I]
_lib.q3t_synchronize.argtypes = [_P]
_lib.q3t_last_timing.argtypes = [_P, C.POINTER(C.c_double), C.POINTER(C.c_double)]
_lib.q3t_time_stage.argtypes = [_P, _I, _I, _I, _I, C.POINTER(C.c_double)]
_lib.q3t_persist_status.argtypes = [_P]
_lib.q3t_persist_kernels.argtypes = [_P]
_lib.q3t_decode_family.argtypes = [_P, _I]
if hasattr(_lib, "q3t_debug_read"):   # development builds only (make -C csrc DEV=1)
    _lib.q3t_debug_read.argtypes = [_P, _I, _P, C.c_size_t]
_lib.q3t_vocoder_num_samples.restype = C.c_int64
_lib.q3t_vocoder_num_samples.argtypes = [_P, C.c_int32, _I]
_lib.q3t_vocoder_flops.restype = C.c_double
_lib.q3t_vocoder_flops.argtypes = [_P, C.c_int32]
_lib.q3t_vocoder_decode.argtypes = [_P, _ip, C.c_int32, _I, _fp, C.POINTER(C.c_int64)]
_lib.q3t_vocoder_decode_chunked.argtypes = [_P, _ip, C.c_int32, C.c_int32, C.c_int32, _fp, C.POINTER(C.c_int64)]
_lib.q3t_vocoder_decode_batch.argtypes = [_P, C.c_int32, C.POINTER(C.c_void_p), _ip, _I, C.c_int32,
                                          C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
_lib.q3t_vocoder_set_batch_frames.argtypes = [_P, C.c_int32]
_lib.q3t_vocoder_stream_open.argtypes = [_P, C.c_int32, C.POINTER(_P)]
_lib.q3t_vocoder_stream_push.argtypes = [_P, _P, C.c_int32, _P, C.c_int64, C.POINTER(C.c_int64)]
_lib.q3t_vocoder_stream_push_batch.argtypes = [_P, C.c_int32, _P, _P, _P, _P, _P]
_lib.q3t_vocoder_stream_last_groups.restype = C.c_int32
_lib.q3t_vocoder_stream_last_groups.argtypes = [_P]
_lib.q3t_vocoder_stream_samples.restype = C.c_int64
_lib.q3t_vocoder_stream_samples.argtypes = [_P]
_lib.q3t_vocoder_stream_frames.restype = C.c_int32
_lib.q3t_vocoder_stream_frames.argtypes = [_P]
_lib.q3t_vocoder_stream_halo.restype = C.c_int32
_lib.q3t_vocoder_stream_halo.argtypes = [_P]
_lib.q3t_vocoder_stream_reset.argtypes = [_P]
_lib.q3t_pcm_bytes_per_sample.restype = C.c_int32
_lib.q3t_pcm_bytes_per_sample.argtypes = [C.c_int32]
_lib.q3t_pcm_num_samples.restype = C.c_int64
_lib.q3t_pcm_num_samples.argtypes = [C.c_int64, C.c_int32, C.c_int32]
_lib.q3t_pcm_taps.argtypes = [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P, C.c_int64]
_lib.q3t_vocoder_decode_out.argtypes = [_P, _ip, C.c_int32, _I, _P, _P, C.c_int64, C.POINTER(C.c_int64)]
_lib.q3t_vocoder_stream_set_output.argtypes = [_P, _P]
_lib.q3t_vocoder_stream_push_out.argtypes = [_P, _P, C.c_int32, C.c_int32, _P, C.c_int64, C.POINTER(C.c_int64)]
_lib.q3t_vocoder_stream_push_batch_out.argtypes = [_P, C.c_int32, _P, _P, _P, _P, _P, _P]
_lib.q3t_vocoder_stream_out_samples.restype = C.c_int64
_lib.q3t_vocoder_stream_out_samples.argtypes = [_P]
_lib.q3t_pcm_out_launches.restype = C.c_int64
_lib.q3t_pcm_out_launches.argtypes = []
_lib.q3t_vocoder_stream_close.restype = None
_lib.q3t_vocoder_stream_close.argtypes = [_P]
_lib.q3t_speaker_dim.argtypes = [_P]
_lib.q3t_ctx_create_speaker.argtypes = [C.c_char_p, _I, C.POINTER(_P)]
_lib.q3t_speaker_encode.argtypes = [_P, _fp, C.c_int32, _fp]
_lib.q3t_speaker_encode_batch.argtypes = [_P, C.POINTER(C.POINTER(C.c_float)), _ip, C.c_int32, _fp, _P]
_lib.q3t_speaker_launches.restype = C.c_int64
_lib.q3t_speaker_launches.argtypes = []
_lib.q3t_speaker_mel.argtypes = [_P, _fp, C.c_int32, _P, C.c_int32, C.POINTER(C.c_int32)]
_lib.q3t_tokenizer_load.argtypes = [C.c_char_p, C.POINTER(_P)]
_lib.q3t_tokenizer_free.argtypes = [_P]
_lib.q3t_tokenizer_info.argtypes = [_P] + [C.POINTER(C.c_int32)] * 4
_lib.q3t_tokenizer_encode.argtypes = [_P, C.c_char_p, C.c_int64, _I, _P, C.c_int32, C.POINTER(C.c_int32)]
_lib.q3t_tokenizer_decode.argtypes = [_P, _P, C.c_int32, _P, C.c_int64, C.POINTER(C.c_int64)]
_lib.q3t_talker_forward.argtypes = [_P, _I, _fp, _ip, _P, _P]
_lib.q3t_talker_prefill.argtypes = [_P, _I, _I, _fp, _I, _P, _P]
_lib.q3t_codepred_frame.argtypes = [_P, _I, _fp, _ip, _F, C.c_int32, C.c_uint64, C.c_int32, _ip, _P]
_lib.q3t_cb0_select.argtypes = [_P, _I, _fp, np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS"), _ip, _ip,
                                C.POINTER(GenParams), _ip]
_lib.q3t_project_text.argtypes = [_P, _I, _ip, _fp]
_lib.q3t_prefill_embd.argtypes = [_P, _ip, _I, _P, _I, _fp, C.POINTER(C.c_int32), _fp, C.POINTER(C.c_int32), _fp]

# names the C ABI must export (checked by tests without a GPU)
EXPORTS = ["q3t_last_error", "q3t_default_params", "q3t_ctx_create", "q3t_ctx_destroy", "q3t_get_config",
           "q3t_generate", "q3t_generate_stream", "q3t_generate_queue", "q3t_generate_queue_stream", "q3t_comm_unique_id", "q3t_ctx_create_shared",
           "q3t_plan_weight_layout", "q3t_ctx_create_replica", "q3t_comm_allreduce_max", "q3t_set_mfma_min_batch", "q3t_synchronize", "q3t_last_timing", "q3t_time_stage", "q3t_persist_status", "q3t_persist_kernels", "q3t_decode_family", "q3t_vocoder_num_samples", "q3t_vocoder_flops", "q3t_vocoder_decode",
           "q3t_vocoder_decode_chunked", "q3t_vocoder_decode_batch", "q3t_vocoder_set_batch_frames",
           "q3t_vocoder_stream_open", "q3t_vocoder_stream_push", "q3t_vocoder_stream_push_batch",
           "q3t_vocoder_stream_last_groups", "q3t_vocoder_stream_samples",
           "q3t_vocoder_stream_frames", "q3t_vocoder_stream_halo", "q3t_vocoder_stream_close", "q3t_vocoder_stream_reset", "q3t_speaker_dim", "q3t_ctx_create_speaker", "q3t_speaker_encode", "q3t_speaker_mel",
           "q3t_speaker_encode_batch", "q3t_speaker_launches",
           "q3t_tokenizer_load", "q3t_tokenizer_free", "q3t_tokenizer_info", "q3t_tokenizer_encode",
           "q3t_tokenizer_decode", "q3t_talker_forward", "q3t_talker_prefill", "q3t_talker_prefill_ragged",
           "q3t_utt_params_from", "q3t_generate_utt", "q3t_generate_queue_utt", "q3t_generate_queue_text",
           "q3t_text_feed_stats", "q3t_generate_queue_open", "q3t_check_utt",
           "q3t_pcm_bytes_per_sample", "q3t_pcm_num_samples", "q3t_pcm_taps", "q3t_vocoder_decode_out",
           "q3t_vocoder_stream_set_output", "q3t_vocoder_stream_push_out", "q3t_vocoder_stream_push_batch_out",
           "q3t_vocoder_stream_out_samples", "q3t_pcm_out_launches",
           "q3t_codepred_frame", "q3t_cb0_select", "q3t_project_text", "q3t_prefill_embd", "gpu_fp32_to_fp16",
           "gpu_argmax_f32", "gpu_embedding_lookup_by_gpu_id", "gpu_sample_topk_f32"]


def lib():
    return _lib


def _check(rc):
    if rc != 0:
        raise Q3TError(_lib.q3t_last_error().decode(errors="replace"))


def default_params(**kw):
    p = GenParams()
    _lib.q3t_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


_UTT_KEYS = ("language_id", "max_len", "repetition_penalty", "temperature", "top_k", "force_frames")


def utt_params(p, per_utt, n):
    """The q3t_utt_params array of a call: the call's values (GenParams p) with each utterance's overrides
    (per_utt[u]: a dict over language_id / max_len / repetition_penalty / temperature / top_k / force_frames, or None)."""
    if len(per_utt) != n:
        raise ValueError("per_utt: one entry (a dict or None) per prompt")
    up = (UttParams * n)()
    for u in range(n):
        _lib.q3t_utt_params_from(C.byref(p), C.byref(up[u]))
        for k, v in (per_utt[u] or {}).items():
            if k not in _UTT_KEYS:
                raise ValueError(f"per_utt[{u}]: unknown key {k!r} (per utterance: {', '.join(_UTT_KEYS)})")
            setattr(up[u], k, v)
    return up


def _speaker_array(speakers, n, optional):
    """(pointer array or None, the arrays it points into); optional: entries may be None (per-utterance calls)"""
    if speakers is None:
        return None, []
    if len(speakers) != n:
        raise ValueError("one speaker embedding per prompt, or none")
    if not optional and any(s is None for s in speakers):
        raise ValueError("a speaker entry may be None only with per_utt")
    sp = [None if s is None else np.ascontiguousarray(s, np.float32) for s in speakers]
    null = C.POINTER(C.c_float)()
    return (C.POINTER(C.c_float) * n)(*[null if s is None else s.ctypes.data_as(C.POINTER(C.c_float)) for s in sp]), sp


def _check_frames(rc, nf):
    """_check whose error carries the call's n_frames (all zero after a validation failure)"""
    if rc != 0:
        e = Q3TError(_lib.q3t_last_error().decode(errors="replace"))
        e.n_frames = [int(x) for x in nf]
        raise e


def _addr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _queue_cb(on_batch, errors):
    """q3t_queue_cb over on_batch(entries) (Engine.generate_queue_stream); an exception ends the call and lands in errors"""
    def _cb(_user, m, utt, cptr, nfr, fin, stop):
        try:
            entries = []
            for i in range(m):
                k = int(nfr[i])
                arr = (np.ctypeslib.as_array(cptr[i], shape=(k * 16,)).reshape(k, 16).copy() if k > 0
                       else np.zeros((0, 16), np.int32))
                entries.append((int(utt[i]), arr, bool(fin[i])))
            r = on_batch(entries)
            if r is False:
                return 0
            if r is not None and r is not True:
                where = {int(utt[i]): i for i in range(m)}
                for u in r:
                    if int(u) in where:
                        stop[where[int(u)]] = 1
            return 1
        except Exception as e:  # never let an exception unwind through the C frames
            errors.append(e)
            return 0

    return QUEUE_CB(_cb)


def set_mfma_min_batch(b):
    """Process-wide: batches of >= b slots use the matrix-core GEMM (0 = never).  Affects contexts created later."""
    _check(_lib.q3t_set_mfma_min_batch(int(b)))


def comm_unique_id():
    """RCCL unique id (rank 0), Q3T_COMM_ID_BYTES bytes to hand to every rank of q3t_ctx_create_shared."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(_lib.q3t_comm_unique_id(buf))
    return buf.raw


def plan_weight_layout(tts_gguf):
    """Host-only weight layout of a model file (no device): (byte offset of every allocation of the talker blob in
    order, bytes used) -- what each rank of a shared start-up computes from the GGUF headers before the broadcast."""
    n = C.c_int(0)
    used = C.c_uint64(0)
    _check(_lib.q3t_plan_weight_layout(str(tts_gguf).encode(), None, 0, C.byref(n), C.byref(used)))
    off = np.zeros(max(n.value, 1), np.uint64)
    _check(_lib.q3t_plan_weight_layout(str(tts_gguf).encode(), _addr(off), n.value, C.byref(n), C.byref(used)))
    return off[:n.value], int(used.value)


class Tokenizer:
    """TextTokenizer (src/text_tokenizer.h): byte-level BPE + the TTS template, read from the TTS GGUF.  Host only."""

    def __init__(self, gguf_path):
        h = _P()
        _check(_lib.q3t_tokenizer_load(gguf_path.encode(), C.byref(h)))
        self.h = h
        v, b, e, p = (C.c_int32() for _ in range(4))
        _check(_lib.q3t_tokenizer_info(self.h, C.byref(v), C.byref(b), C.byref(e), C.byref(p)))
        self.vocab_size, self.bos, self.eos, self.pad = v.value, b.value, e.value, p.value

    def close(self):
        if getattr(self, "h", None):
            _lib.q3t_tokenizer_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def encode(self, text, for_tts=False):
        raw = text.encode("utf-8", errors="surrogateescape") if isinstance(text, str) else bytes(text)
        n = C.c_int32(0)
        _check(_lib.q3t_tokenizer_encode(self.h, raw, len(raw), int(bool(for_tts)), None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), np.int32)
        _check(_lib.q3t_tokenizer_encode(self.h, raw, len(raw), int(bool(for_tts)), _addr(out), n.value, C.byref(n)))
        return out[:n.value].tolist()

    def encode_for_tts(self, text):
        return self.encode(text, for_tts=True)

    def decode(self, ids):
        """bytes of the decoded text"""
        a = np.ascontiguousarray(ids, np.int32)
        nb = C.c_int64(0)
        _check(_lib.q3t_tokenizer_decode(self.h, _addr(a), len(a), None, 0, C.byref(nb)))
        buf = C.create_string_buffer(max(nb.value, 1))
        _check(_lib.q3t_tokenizer_decode(self.h, _addr(a), len(a), buf, nb.value, C.byref(nb)))
        return buf.raw[:nb.value]


class TextFeeder:
    """Text that arrives in pieces -> token ids whose concatenation is Tokenizer.encode(whole text), however the text
    was cut (the ids Engine.generate_queue_text's text_source feeds).  The tokenizer starts a word at every space and
    keeps the space with the word, so what follows the last space is held back until more text arrives or close()."""

    def __init__(self, tokenizer):
        self.tok = tokenizer
        self.pending = b""

    def feed(self, text):
        """ids of the words `text` completes (str, or bytes of UTF-8 text cut anywhere)"""
        raw = text.encode("utf-8", errors="surrogateescape") if isinstance(text, str) else bytes(text)
        buf = self.pending + raw
        cut = buf.rfind(b" ")   # the word that starts at the last space may still grow
        if cut <= 0:
            self.pending = buf
            return []
        self.pending = buf[cut:]
        return self.tok.encode(buf[:cut])

    def close(self):
        """ids of the held-back rest; the feeder is empty afterwards"""
        buf, self.pending = self.pending, b""
        return self.tok.encode(buf) if buf else []


class ArrivalQueue:
    """A thread-safe source for Engine.generate_queue_open: any thread submit()s requests while the queue runs on
    another; pass its `source` method as the call's source.  Requests are handed over in submission order, so the id
    submit() returns is the id the deliveries name.  The source waits (on a condition) only when the engine says it is
    idle; otherwise it returns at once with what is there and fits."""

    def __init__(self):
        self._cv = threading.Condition()
        self._q = collections.deque()
        self._next = 0
        self._closed = False

    def submit(self, prompt, speaker=None, key=None, **per_utt):
        """queue one request (per_utt: language_id / max_len / repetition_penalty / temperature / top_k /
        force_frames); key: its sampling key (default: its id).  Returns its id."""
        with self._cv:
            if self._closed:
                raise ValueError("ArrivalQueue: submit after close")
            uid = self._next
            self._next += 1
            self._q.append(dict(prompt=prompt, speaker=speaker, key=uid if key is None else key, **per_utt))
            self._cv.notify_all()
            return uid

    def close(self):
        """no more requests: the call returns when the ones submitted have ended"""
        with self._cv:
            self._closed = True
            self._cv.notify_all()

    def source(self, next_id, room, running, idle):
        with self._cv:
            if idle:
                self._cv.wait_for(lambda: self._q or self._closed)
            out = [self._q.popleft() for _ in range(min(room, len(self._q)))]
            return out, self._closed and not self._q


PCM_F32, PCM_S16, PCM_MULAW = 0, 1, 2
PCM_RATES = (8000, 12000, 16000, 22050, 24000, 32000, 44100, 48000)
_PCM_DTYPES = {PCM_F32: np.float32, PCM_S16: np.int16, PCM_MULAW: np.uint8}


class PcmSpec(C.Structure):
    """q3t_pcm_spec: the output stage's sample rate (one of PCM_RATES) and format (PCM_F32 / PCM_S16 / PCM_MULAW)"""
    _fields_ = [("sample_rate", C.c_int32), ("format", C.c_int32)]

    @classmethod
    def of(cls, out):
        """a PcmSpec, or (rate, format)"""
        return out if isinstance(out, cls) else cls(int(out[0]), int(out[1]))

    @property
    def dtype(self):
        return _PCM_DTYPES.get(self.format, np.uint8)


def pcm_num_samples(n_in_total, sample_rate, final=False):
    """output samples after n_in_total vocoder samples (final: with the filter's tail); -1 for an unsupported rate"""
    return _lib.q3t_pcm_num_samples(int(n_in_total), int(sample_rate), 1 if final else 0)


def pcm_taps(sample_rate):
    """(L, M, K, taps [L][K] float32): the polyphase geometry and the exact tap table of the output stage's kernel"""
    L, M, K = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _check(_lib.q3t_pcm_taps(int(sample_rate), C.byref(L), C.byref(M), C.byref(K), None, 0))
    taps = np.zeros((L.value, K.value), np.float32)
    _check(_lib.q3t_pcm_taps(int(sample_rate), C.byref(L), C.byref(M), C.byref(K), _addr(taps) if taps.size else None, taps.size))
    return L.value, M.value, K.value, taps


class VocoderStream:
    """A streaming FULL vocoder decode (q3t_vocoder_stream_*): push() frames in pieces of any size; the concatenated
    PCM equals Engine.vocoder(all codes) bit for bit.  out=(rate, format) puts the output stage behind it: push()
    then returns float32, int16 or uint8 at that rate, and the concatenation (the last push final) equals
    Engine.vocoder(all codes, out=...) byte for byte.  Closed with the engine at the latest."""

    def __init__(self, engine, max_frames=4096, out=None):
        self.engine = engine
        self.out = None
        h = _P()
        _check(_lib.q3t_vocoder_stream_open(engine.h, int(max_frames), C.byref(h)))
        self.h = h
        engine._streams.add(self)
        if out is not None:
            try:
                self.set_output(out)
            except Q3TError:
                self.close()
                raise

    def set_output(self, out):
        """the output spec (PcmSpec, (rate, format) or None to clear it); only at zero frames"""
        spec = None if out is None else PcmSpec.of(out)
        _check(_lib.q3t_vocoder_stream_set_output(self._handle(), C.byref(spec) if spec is not None else None))
        self.out = spec

    def _out_cap(self, n_frames, final):
        """(samples, bytes) of an output push of n_frames"""
        total = self.engine.vocoder_num_samples(self.frames + n_frames, VOCODER_FULL) if n_frames > 0 else self.samples
        n = max(pcm_num_samples(total, self.out.sample_rate, final) - self.out_samples, 0)
        return n, n * _lib.q3t_pcm_bytes_per_sample(self.out.format)

    def _handle(self):
        if not getattr(self, "h", None) or not self.engine.h:
            raise Q3TError("vocoder stream is closed")
        return self.h

    def push(self, codes, final=False):
        """codes [n][16] int32 -> the next samples: float32 at the vocoder's rate, or the stream's output spec's
        (final: with the filter's tail; the stream then takes no push until reset())"""
        codes = np.ascontiguousarray(codes, np.int32).reshape(-1, 16)
        h, n = self._handle(), codes.shape[0]
        if self.out is not None:
            cnt, nbytes = self._out_cap(n, final)
            buf = np.zeros(max(cnt, 1), self.out.dtype)
            ns = C.c_int64(0)
            _check(_lib.q3t_vocoder_stream_push_out(h, _addr(codes), n, 1 if final else 0, _addr(buf), nbytes, C.byref(ns)))
            return buf[:ns.value]
        if final:
            raise Q3TError("final needs an output spec (the plain stream has no tail to flush)")
        cap = max(self.engine.vocoder_num_samples(self.frames + n, VOCODER_FULL) - self.samples, 0) if n > 0 else 0
        pcm = np.zeros(max(cap, 1), np.float32)
        ns = C.c_int64(0)
        _check(_lib.q3t_vocoder_stream_push(h, _addr(codes), n, _addr(pcm), cap, C.byref(ns)))
        return pcm[:ns.value]

    def reset(self):
        """back to zero frames and zero samples, keeping the caches: the next pushes equal a fresh stream's"""
        _check(_lib.q3t_vocoder_stream_reset(self._handle()))

    @property
    def frames(self):
        return _lib.q3t_vocoder_stream_frames(self._handle())

    @property
    def samples(self):
        return _lib.q3t_vocoder_stream_samples(self._handle())

    @property
    def out_samples(self):
        """output samples so far (-1 without an output spec)"""
        return _lib.q3t_vocoder_stream_out_samples(self._handle())

    @property
    def halo(self):
        return _lib.q3t_vocoder_stream_halo(self._handle())

    def close(self):
        if getattr(self, "h", None):
            if self.engine.h:   # a destroyed context has already freed its streams
                _lib.q3t_vocoder_stream_close(self.h)
            self.h = None
            self.engine._streams.discard(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine:
    """One device context (TTSTransformer + code predictor + vocoder resident in HBM)."""

    def __init__(self, tts_gguf=None, tokenizer_gguf=None, device=0, max_slots=1, max_ctx=4096 + 32, *, _handle=None):
        if _handle is None:
            h = _P()
            _check(_lib.q3t_ctx_create(tts_gguf.encode() if tts_gguf else None,
                                       tokenizer_gguf.encode() if tokenizer_gguf else None,
                                       int(device), int(max_slots), int(max_ctx), C.byref(h)))
            _handle = h
        self.h = _handle
        self._streams = weakref.WeakSet()   # open VocoderStreams (the context frees them when it is destroyed)
        c = Config()
        _check(_lib.q3t_get_config(self.h, C.byref(c)))
        self.cfg = {n: getattr(c, n) for n, _ in Config._fields_}

    @classmethod
    def shared(cls, tts_gguf, tokenizer_gguf, device, max_slots, max_ctx, rank, world, uid):
        """One rank of a multi-GPU job: rank 0 reads the weights, RCCL broadcasts them to the others."""
        assert len(uid) == COMM_ID_BYTES
        h = _P()
        _check(_lib.q3t_ctx_create_shared(tts_gguf.encode(), tokenizer_gguf.encode() if tokenizer_gguf else None,
                                          int(device), int(max_slots), int(max_ctx), int(rank), int(world), uid,
                                          C.byref(h)))
        return cls(_handle=h)

    @classmethod
    def speaker_only(cls, tts_gguf, device=0):
        """a context with only the speaker encoder loaded (AudioTokenizerEncoder::load_model)"""
        h = _P()
        _check(_lib.q3t_ctx_create_speaker(tts_gguf.encode(), int(device), C.byref(h)))
        return cls(_handle=h)

    def replica(self, device=0, max_slots=1, max_ctx=4096 + 32):
        """A second context whose weights are copied device-to-device from this one (no file reads)."""
        h = _P()
        _check(_lib.q3t_ctx_create_replica(self.h, int(device), int(max_slots), int(max_ctx), C.byref(h)))
        return Engine(_handle=h)

    def allreduce_max(self, values):
        v = np.ascontiguousarray(values, np.float64).copy()
        _check(_lib.q3t_comm_allreduce_max(self.h, v, len(v)))
        return v

    def close(self):
        if getattr(self, "h", None):
            for st in list(getattr(self, "_streams", [])):
                st.close()
            _lib.q3t_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- hot path
    def generate(self, prompts, speakers=None, per_utt=None, **params):
        """prompts: list of token-id lists.  Returns list of [n_frames][16] int32 arrays.
        per_utt: one dict (or None) per prompt overriding the call's language_id / max_len / repetition_penalty /
        temperature / top_k / force_frames for that utterance (q3t_generate_utt); speakers may then hold None entries.
        The seed and the call's max_len (the cap of every per-utterance max_len) stay per call."""
        p = default_params(**params)
        n = len(prompts)
        if per_utt is not None:
            return self._generate_utt(prompts, speakers, per_utt, p, None, 0)
        toks = [np.ascontiguousarray(t, np.int32) for t in prompts]
        tarr = (C.POINTER(C.c_int32) * n)(*[t.ctypes.data_as(C.POINTER(C.c_int32)) for t in toks])
        ntok = np.array([len(t) for t in toks], np.int32)
        sarr = None
        keep = []
        if speakers is not None:
            sp = [np.ascontiguousarray(s, np.float32) for s in speakers]
            keep = sp
            sarr = (C.POINTER(C.c_float) * n)(*[s.ctypes.data_as(C.POINTER(C.c_float)) for s in sp])
        codes = np.zeros((n, p.max_len, 16), np.int32)
        nf = np.zeros(n, np.int32)
        _check(_lib.q3t_generate(self.h, n, tarr, ntok, sarr, C.byref(p), codes, nf))
        del keep
        return [codes[i, :nf[i]].copy() for i in range(n)]

    def _generate_utt(self, prompts, speakers, per_utt, p, cb, interval):
        n = len(prompts)
        up = utt_params(p, per_utt, n)
        toks = [np.ascontiguousarray(t, np.int32) for t in prompts]
        tarr = (C.POINTER(C.c_int32) * n)(*[t.ctypes.data_as(C.POINTER(C.c_int32)) for t in toks])
        ntok = np.array([len(t) for t in toks], np.int32)
        sarr, keep = _speaker_array(speakers, n, True)
        codes = np.zeros((n, p.max_len, 16), np.int32)
        nf = np.zeros(n, np.int32)
        _check_frames(_lib.q3t_generate_utt(self.h, n, tarr, ntok, sarr, C.byref(p), up, codes, nf,
                                            C.cast(cb, C.c_void_p) if cb else None, None, int(interval)), nf)
        del keep
        return [codes[i, :nf[i]].copy() for i in range(n)]

    def _generate_queue_utt(self, prompts, speakers, per_utt, p, max_active, cb, interval, want_codes):
        n = len(prompts)
        up = utt_params(p, per_utt, n)
        toks = [np.ascontiguousarray(t, np.int32) for t in prompts]
        tarr = (C.POINTER(C.c_int32) * n)(*[t.ctypes.data_as(C.POINTER(C.c_int32)) for t in toks])
        ntok = np.array([len(t) for t in toks], np.int32)
        sarr, keep = _speaker_array(speakers, n, True)
        codes = np.zeros((n, p.max_len, 16), np.int32) if want_codes else None
        nf = np.zeros(n, np.int32)
        _check_frames(_lib.q3t_generate_queue_utt(self.h, n, tarr, ntok, sarr, C.byref(p), up, _addr(codes), nf,
                                                  int(max_active), C.cast(cb, C.c_void_p) if cb else None, None,
                                                  int(interval)), nf)
        del keep
        if not want_codes:
            return [int(x) for x in nf]
        return [codes[i, :nf[i]].copy() for i in range(n)]

    def generate_queue(self, prompts, speakers=None, max_active=0, per_utt=None, **params):
        """continuous batching (q3t_generate_queue): any number of prompts through the context's slots, a finished
        utterance's slot refilled with the next prompt.  Returns list of [n_frames][16] int32 arrays.
        per_utt: as in generate() (q3t_generate_queue_utt)."""
        p = default_params(**params)
        n = len(prompts)
        if per_utt is not None:
            return self._generate_queue_utt(prompts, speakers, per_utt, p, max_active, None, 0, True)
        toks = [np.ascontiguousarray(t, np.int32) for t in prompts]
        tarr = (C.POINTER(C.c_int32) * n)(*[t.ctypes.data_as(C.POINTER(C.c_int32)) for t in toks])
        ntok = np.array([len(t) for t in toks], np.int32)
        sarr = None
        keep = []
        if speakers is not None:
            sp = [np.ascontiguousarray(s, np.float32) for s in speakers]
            keep = sp
            sarr = (C.POINTER(C.c_float) * n)(*[s.ctypes.data_as(C.POINTER(C.c_float)) for s in sp])
        codes = np.zeros((n, p.max_len, 16), np.int32)
        nf = np.zeros(n, np.int32)
        _check(_lib.q3t_generate_queue(self.h, n, tarr, ntok, sarr, C.byref(p), codes, nf, int(max_active)))
        del keep
        return [codes[i, :nf[i]].copy() for i in range(n)]

    def generate_stream(self, prompts, on_frames, interval=40, speakers=None, per_utt=None, **params):
        """generate() with the reference's frame callback: on_frames(utt, codes [n][16]) -> bool, every `interval`
        frames plus a final flush; returning False stops that utterance.  Returns the codes like generate().
        per_utt: as in generate()."""
        p = default_params(**params)
        n = len(prompts)
        errors = []

        def _cb(_user, utt, ptr, nfr, ncb):
            try:
                arr = np.ctypeslib.as_array(ptr, shape=(nfr * ncb,)).reshape(nfr, ncb).copy()
                return 1 if on_frames(int(utt), arr) is not False else 0
            except Exception as e:  # never let an exception unwind through the C frames
                errors.append(e)
                return 0

        cb = FRAME_CB(_cb)
        if per_utt is not None:
            out = self._generate_utt(prompts, speakers, per_utt, p, cb, interval)
            if errors:
                raise errors[0]
            return out
        toks = [np.ascontiguousarray(t, np.int32) for t in prompts]
        tarr = (C.POINTER(C.c_int32) * n)(*[t.ctypes.data_as(C.POINTER(C.c_int32)) for t in toks])
        ntok = np.array([len(t) for t in toks], np.int32)
        sarr = None
        sp = []
        if speakers is not None:
            sp = [np.ascontiguousarray(s, np.float32) for s in speakers]
            sarr = (C.POINTER(C.c_float) * n)(*[s.ctypes.data_as(C.POINTER(C.c_float)) for s in sp])
        codes = np.zeros((n, p.max_len, 16), np.int32)
        nf = np.zeros(n, np.int32)
        _check(_lib.q3t_generate_stream(self.h, n, tarr, ntok, sarr, C.byref(p), codes, nf, cb, None, int(interval)))
        del sp
        if errors:
            raise errors[0]
        return [codes[i, :nf[i]].copy() for i in range(n)]

    def generate_queue_stream(self, prompts, on_batch, interval=12, speakers=None, max_active=0, want_codes=True,
                              per_utt=None, **params):
        """generate_queue() that hands frames out while it runs (q3t_generate_queue_stream).  on_batch(entries) is
        called once per tick (every `interval` frames of the queue's loop) or finish with a list of
        (utt, codes [n][16] int32, final); it returns None or True to continue, an iterable of utterance indices to
        cancel, or False to abort the call.  Per utterance the pieces arrive in order, concatenate to generate_queue's
        codes, and exactly one is final.  Returns the codes like generate_queue() (a cancelled utterance: the frames
        it was handed), or with want_codes=False (no code buffers kept) the list of frame counts.
        per_utt: as in generate(); no piece reaches beyond an utterance's own max_len."""
        if not callable(on_batch):
            raise TypeError("generate_queue_stream: on_batch must be callable (use generate_queue without one)")
        if isinstance(interval, bool) or not isinstance(interval, (int, np.integer)) or interval <= 0:
            raise ValueError("generate_queue_stream: interval must be an integer > 0")
        if speakers is not None and len(speakers) != len(prompts):
            raise ValueError("generate_queue_stream: one speaker embedding per prompt, or none")
        p = default_params(**params)
        n = len(prompts)
        errors = []
        cb = _queue_cb(on_batch, errors)
        if per_utt is not None:
            out = self._generate_queue_utt(prompts, speakers, per_utt, p, max_active, cb, interval, want_codes)
            if errors:
                raise errors[0]
            return out
        toks = [np.ascontiguousarray(t, np.int32) for t in prompts]
        tarr = (C.POINTER(C.c_int32) * n)(*[t.ctypes.data_as(C.POINTER(C.c_int32)) for t in toks])
        ntok = np.array([len(t) for t in toks], np.int32)
        sarr = None
        sp = []
        if speakers is not None:
            sp = [np.ascontiguousarray(s, np.float32) for s in speakers]
            sarr = (C.POINTER(C.c_float) * n)(*[s.ctypes.data_as(C.POINTER(C.c_float)) for s in sp])
        codes = np.zeros((n, p.max_len, 16), np.int32) if want_codes else None
        nf = np.zeros(n, np.int32)
        _check(_lib.q3t_generate_queue_stream(self.h, n, tarr, ntok, sarr, C.byref(p), _addr(codes) if want_codes else None,
                                              nf, int(max_active), cb, None, int(interval)))
        del sp
        if errors:
            raise errors[0]
        if not want_codes:
            return [int(x) for x in nf]
        return [codes[i, :nf[i]].copy() for i in range(n)]

    def generate_queue_text(self, prompts, open, text_source, on_batch=None, interval=12, speakers=None, max_active=0,
                            per_utt=None, **params):
        """generate_queue() whose utterances may be fed their text while they speak (q3t_generate_queue_text).
        open[u] true: prompts[u] is a head -- the three role ids and at least one text id, without the five-id suffix
        of a whole prompt -- and its further text ids come from text_source(utt, frames, rows_ahead) -> (ids, end):
        frames = the frames the utterance has generated, rows_ahead = the frames it can still run before it is held;
        end true closes the text after ids.  (None or () stands for ([], False); returning False aborts the call.)
        It is asked when the utterance takes a slot, every `interval` frames of the queue's loop, and again and again
        while the utterance has no row for its next frame: blocking until text exists is its job.  The codes are those
        of generate_queue() for head + fed ids + five ids, however the ids were cut.
        on_batch: as in generate_queue_stream() (an open utterance's pieces may be shorter than `interval`).
        Returns (codes list, held list): held[u] = how often utterance u was put on hold."""
        if isinstance(interval, bool) or not isinstance(interval, (int, np.integer)) or interval <= 0:
            raise ValueError("generate_queue_text: interval must be an integer > 0")
        n = len(prompts)
        if len(open) != n:
            raise ValueError("generate_queue_text: one open flag per prompt")
        if on_batch is not None and not callable(on_batch):
            raise TypeError("generate_queue_text: on_batch must be callable or None")
        p = default_params(**params)
        errors = []
        keep_ids = []   # the array handed to the C side stays alive until the next ask

        def _text(_user, utt, frames, ahead, ids_out, n_out, end_out):
            try:
                r = text_source(int(utt), int(frames), int(ahead))
                if r is False:
                    return 0
                ids, end = r if r else ((), False)
                a = np.ascontiguousarray(ids, np.int32).reshape(-1)
                keep_ids[:] = [a]
                ids_out[0] = a.ctypes.data_as(C.POINTER(C.c_int32))
                n_out[0] = len(a)
                end_out[0] = 1 if end else 0
                return 1
            except Exception as e:  # never let an exception unwind through the C frames
                errors.append(e)
                return 0

        tcb = TEXT_CB(_text) if text_source is not None else None
        cb = _queue_cb(on_batch, errors) if on_batch is not None else None
        up = utt_params(p, per_utt, n) if per_utt is not None else None
        toks = [np.ascontiguousarray(t, np.int32) for t in prompts]
        tarr = (C.POINTER(C.c_int32) * n)(*[t.ctypes.data_as(C.POINTER(C.c_int32)) for t in toks])
        ntok = np.array([len(t) for t in toks], np.int32)
        sarr, keep = _speaker_array(speakers, n, per_utt is not None)
        flags = np.ascontiguousarray([1 if o else 0 for o in open], np.uint8)
        codes = np.zeros((n, p.max_len, 16), np.int32)
        nf = np.zeros(n, np.int32)
        held = np.zeros(n, np.int32)
        rc = _lib.q3t_generate_queue_text(self.h, n, tarr, ntok, sarr, C.byref(p), C.cast(up, C.c_void_p) if up else None,
                                          _addr(flags), _addr(codes), nf, _addr(held), int(max_active),
                                          C.cast(cb, C.c_void_p) if cb else None, None, int(interval),
                                          C.cast(tcb, C.c_void_p) if tcb else None, None)
        del keep
        if errors:
            raise errors[0]
        _check_frames(rc, nf)
        return [codes[i, :nf[i]].copy() for i in range(n)], [int(x) for x in held]

    def generate_queue_open(self, source, on_batch, interval=12, slots=0, max_active=0, **params):
        """The open queue (q3t_generate_queue_open): utterances are admitted while continuous batching runs.
        source(next_id, room, running, idle) -> (list of dict(prompt=, speaker=, key=, **per_utt), closed) is asked
        between two frames whenever a slot could take a newcomer; it returns at most `room` requests (the first gets
        id next_id) and must return at once unless idle is true, when it may block until a request exists.  closed true:
        no more will come; the call returns when every accepted utterance has ended.  None stands for ([], False),
        returning False aborts the call.  key (default: the id) is the sampling key: the utterance's codes are those of
        index `key` of generate_queue(per_utt=...) at the same slot count, seed and max_len.  on_batch: as in
        generate_queue_stream(), with the ids in place of the indices.  q3t.ArrivalQueue is a ready-made source.
        params: max_len and seed, and the defaults of the per-utterance values.  Returns (n_arrived, n_finished)."""
        if not callable(source) or not callable(on_batch):
            raise TypeError("generate_queue_open: source and on_batch must be callable")
        if isinstance(interval, bool) or not isinstance(interval, (int, np.integer)) or interval <= 0:
            raise ValueError("generate_queue_open: interval must be an integer > 0")
        p = default_params(**params)
        errors = []
        keep = []   # what the records point into stays alive until the next ask

        def _arrive(_user, next_id, room, running, idle, out, n_out, closed_out):
            try:
                r = source(int(next_id), int(room), int(running), bool(idle))
                if r is False:
                    return 0
                items, closed = r if r else ((), False)
                items = list(items)
                keep.clear()
                for i, it in enumerate(items[:room]):
                    it = dict(it)
                    tok = np.ascontiguousarray(it.pop("prompt"), np.int32).reshape(-1)
                    spk = it.pop("speaker", None)
                    key = it.pop("key", None)
                    up = utt_params(p, [it], 1)
                    keep.append(tok)
                    out[i].tokens = tok.ctypes.data_as(C.POINTER(C.c_int32))
                    out[i].n_tokens = len(tok)
                    if spk is None:
                        out[i].speaker = C.POINTER(C.c_float)()
                    else:
                        spk = np.ascontiguousarray(spk, np.float32).reshape(-1)
                        if len(spk) != self.cfg["hidden"]:
                            raise ValueError(f"utterance {next_id + i}: a speaker embedding has {self.cfg['hidden']} floats")
                        keep.append(spk)
                        out[i].speaker = spk.ctypes.data_as(C.POINTER(C.c_float))
                    out[i].up = up[0]
                    out[i].key = int(next_id + i if key is None else key)
                n_out[0] = len(items)   # (more than room: the engine refuses the answer)
                closed_out[0] = 1 if closed else 0
                return 1
            except Exception as e:  # never let an exception unwind through the C frames
                errors.append(e)
                return 0

        acb = ARRIVE_CB(_arrive)
        cb = _queue_cb(on_batch, errors)
        na, nfin = C.c_int32(0), C.c_int32(0)
        rc = _lib.q3t_generate_queue_open(self.h, C.byref(p), int(slots), int(max_active), acb, cb, None, int(interval),
                                          C.byref(na), C.byref(nfin))
        keep.clear()
        if errors:
            raise errors[0]
        _check(rc)
        return na.value, nfin.value

    def check_utt(self, prompt, speaker=None, per_utt=None, **params):
        """What generate_queue_open (or generate_queue with per_utt) would refuse of one request (q3t_check_utt): the
        message, or None if it is fine.  Nothing runs."""
        p = default_params(**params)
        up = utt_params(p, [per_utt], 1)
        tok = np.ascontiguousarray(prompt, np.int32).reshape(-1)
        spk = None if speaker is None else np.ascontiguousarray(speaker, np.float32).reshape(-1)
        rc = _lib.q3t_check_utt(self.h, _addr(tok), len(tok), _addr(spk), C.byref(p), up)
        return None if rc == 0 else _lib.q3t_last_error().decode(errors="replace")

    def text_feed_stats(self):
        """counters of the last generate_queue_text() with an open utterance: frame graphs launched, loop rounds that
        launched none (every busy slot held), feed rounds, and the device time of the feed rounds in ms"""
        a, b, c = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        ms = C.c_double(0)
        _check(_lib.q3t_text_feed_stats(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(ms)))
        return dict(graph_launches=a.value, idle_rounds=b.value, feed_rounds=c.value, feed_ms=ms.value)

    def synchronize(self):
        _check(_lib.q3t_synchronize(self.h))

    def last_timing(self):
        a, b = C.c_double(0), C.c_double(0)
        _check(_lib.q3t_last_timing(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def time_stage(self, stage, n_slots, pos, iters):
        ms = C.c_double(0)
        _check(_lib.q3t_time_stage(self.h, int(stage), int(n_slots), int(pos), int(iters), C.byref(ms)))
        return ms.value

    def persist_status(self):
        """-1: single-slot path runs launch-per-phase; 0: persistent launches in use; 1: one flagged a hand-off
        fault; 2: persistent launches disabled after a fault (bit-identical launch-per-op graphs in use)."""
        return _lib.q3t_persist_status(self.h)

    def persist_kernels(self):
        """bit mask of the single-slot persistent kernels in use: 1 talker roles (persist_tk.hip), 2 talker all-role
        (persist.hip), 4 code-predictor roles (persist_cp.hip), 8 code-predictor all-role (persist.hip)"""
        return _lib.q3t_persist_kernels(self.h)

    def decode_family(self, n_slots):
        """what a frame loop of n_slots slots launches: 0 weight-streaming vector kernels, 1 the launch-per-op
        matrix-core stack, 2 the batched persistent launches"""
        f = _lib.q3t_decode_family(self.h, int(n_slots))
        if f < 0:
            raise Q3TError(_lib.q3t_last_error().decode(errors="replace"))
        return f

    def debug_read(self, which, nbytes):
        """development builds only: raw bytes of a device state buffer (0 K, 1 V cache, 2 QKV, 3 attention, 5 timeline)"""
        buf = np.zeros(nbytes, np.uint8)
        _check(_lib.q3t_debug_read(self.h, int(which), _addr(buf), int(nbytes)))
        return buf

    # ---- vocoder
    def vocoder_num_samples(self, n_frames, mode=VOCODER_FULL):
        return _lib.q3t_vocoder_num_samples(self.h, int(n_frames), int(mode))

    def vocoder_flops(self, n_frames):
        """algorithmic FLOPs of one FULL decode of n_frames"""
        return _lib.q3t_vocoder_flops(self.h, int(n_frames))

    def vocoder(self, codes, mode=VOCODER_FULL, out=None):
        """PCM of codes [n][16]: float32 at the vocoder's rate, or with out=(rate, format) / a PcmSpec the output
        stage's float32 / int16 / uint8 at that rate (q3t_vocoder_decode_out, the filter's tail included)"""
        codes = np.ascontiguousarray(codes, np.int32).reshape(-1, 16)
        n = self.vocoder_num_samples(codes.shape[0], mode)
        if n < 0:
            raise Q3TError("vocoder not loaded")
        if out is not None:
            spec = PcmSpec.of(out)
            cnt = max(pcm_num_samples(n, spec.sample_rate, True), 0)
            buf = np.zeros(max(cnt, 1), spec.dtype)
            ns = C.c_int64(0)
            _check(_lib.q3t_vocoder_decode_out(self.h, codes, codes.shape[0], int(mode), C.byref(spec), _addr(buf),
                                               cnt * buf.itemsize, C.byref(ns)))
            return buf[:ns.value]
        pcm = np.zeros(max(n, 1), np.float32)
        ns = C.c_int64(0)
        _check(_lib.q3t_vocoder_decode(self.h, codes, codes.shape[0], int(mode), pcm, C.byref(ns)))
        return pcm[:ns.value]

    def vocoder_chunked(self, codes, chunk_frames):
        """TRTVocoderDecoder::decode with the engine's fixed_frames (src/trt_vocoder.cpp:98-170)."""
        codes = np.ascontiguousarray(codes, np.int32).reshape(-1, 16)
        pcm = np.zeros(max(codes.shape[0] * 1920, 1), np.float32)
        ns = C.c_int64(0)
        _check(_lib.q3t_vocoder_decode_chunked(self.h, codes, codes.shape[0], 16, int(chunk_frames), pcm, C.byref(ns)))
        return pcm[:ns.value]

    def vocoder_batch(self, codes_list, mode=VOCODER_FULL, chunk_frames=40):
        """several utterances through shared launches (q3t_vocoder_decode_batch): returns one PCM array per
        utterance, each equal to vocoder(codes) (FULL) or vocoder_chunked(codes, chunk_frames) (CHUNK40)"""
        cs = [np.ascontiguousarray(c, np.int32).reshape(-1, 16) for c in codes_list]
        n = len(cs)
        nf = np.array([c.shape[0] for c in cs], np.int32)
        pcms = [np.zeros(max(self.vocoder_num_samples(int(f), mode), 1), np.float32) for f in nf]
        cp = (C.c_void_p * max(n, 1))(*[c.ctypes.data for c in cs])
        pp = (C.c_void_p * max(n, 1))(*[p.ctypes.data for p in pcms])
        ns = (C.c_int64 * max(n, 1))()
        _check(_lib.q3t_vocoder_decode_batch(self.h, n, cp, nf, int(mode), int(chunk_frames), pp, ns))
        return [pcms[i][:ns[i]] for i in range(n)]

    def vocoder_stream(self, max_frames=4096, out=None):
        """a VocoderStream on this context: .push(codes) -> float32 PCM, .frames, .samples, .halo, .close();
        out=(rate, format): .push(codes, final) -> that format at that rate"""
        return VocoderStream(self, max_frames, out)

    def vocoder_stream_push_batch(self, streams, pieces, final=None):
        """one push on each of the VocoderStreams `streams` of this context through shared launches
        (q3t_vocoder_stream_push_batch): pieces[j] is stream j's codes [n_j][16].  Returns the list of each stream's
        next samples (float32), bit-identical to streams[j].push(pieces[j]).  On an error no stream has moved.
        Streams with an output spec (all of the call, or none) go through q3t_vocoder_stream_push_batch_out: each
        returns its own format at its own rate, final[j] ends stream j, and one conversion launch serves them all."""
        streams, pieces = list(streams), list(pieces)
        if len(streams) != len(pieces):
            raise ValueError("one piece of codes per stream")
        k = len(streams)
        codes = [np.ascontiguousarray(p, np.int32).reshape(-1, 16) for p in pieces]
        handles = [st._handle() for st in streams]
        if any(st.out is not None for st in streams):
            fin = [bool(f) for f in final] if final is not None else [False] * k
            if len(fin) != k:
                raise ValueError("one final flag per stream")
            # a stream without a spec among them: sized as f32, refused by the library with its message
            caps = [st._out_cap(c.shape[0], f) if st.out is not None else (0, 0) for st, c, f in zip(streams, codes, fin)]
            bufs = [np.zeros(max(cnt, 1), st.out.dtype if st.out is not None else np.float32)
                    for st, (cnt, _) in zip(streams, caps)]
            harr = (C.c_void_p * k)(*[h.value for h in handles])
            carr = (C.c_void_p * k)(*[c.ctypes.data for c in codes])
            barr = (C.c_void_p * k)(*[b.ctypes.data for b in bufs])
            nf = (C.c_int32 * k)(*[c.shape[0] for c in codes])
            farr = (C.c_int32 * k)(*[1 if f else 0 for f in fin])
            cap = (C.c_int64 * k)(*[nb for _, nb in caps])
            ns = (C.c_int64 * k)()
            _check(_lib.q3t_vocoder_stream_push_batch_out(harr, k, carr, nf, farr, barr, cap, ns))
            return [b[:ns[j]] for j, b in enumerate(bufs)]
        if final is not None and any(final):
            raise Q3TError("final needs an output spec (the plain stream has no tail to flush)")
        caps = [max(self.vocoder_num_samples(st.frames + c.shape[0], VOCODER_FULL) - st.samples, 0) if c.shape[0] > 0 else 0
                for st, c in zip(streams, codes)]
        pcm = [np.zeros(max(cap, 1), np.float32) for cap in caps]
        harr = (C.c_void_p * max(k, 1))(*[h.value for h in handles])
        carr = (C.c_void_p * max(k, 1))(*[c.ctypes.data for c in codes])
        parr = (C.c_void_p * max(k, 1))(*[p.ctypes.data for p in pcm])
        nf = (C.c_int32 * max(k, 1))(*[c.shape[0] for c in codes])
        cap = (C.c_int64 * max(k, 1))(*caps)
        ns = (C.c_int64 * max(k, 1))()
        _check(_lib.q3t_vocoder_stream_push_batch(harr, k, carr, nf, parr, cap, ns))
        return [p[:ns[j]] for j, p in enumerate(pcm)]

    def vocoder_stream_last_groups(self):
        """convolution-stack launch sequences (groups of streams that shared every launch) of the last batched push"""
        return _lib.q3t_vocoder_stream_last_groups(self.h)

    def vocoder_set_batch_frames(self, frames):
        _check(_lib.q3t_vocoder_set_batch_frames(self.h, int(frames)))

    # ---- speaker encoder
    def speaker_dim(self):
        """embedding length of the model's speaker encoder (0: the GGUF has none)"""
        return _lib.q3t_speaker_dim(self.h)

    def encode_speaker(self, samples):
        """AudioTokenizerEncoder::encode (src/audio_tokenizer_encoder.h:107-108): 24 kHz samples in [-1, 1] ->
        speaker embedding [speaker_dim]"""
        x = np.ascontiguousarray(samples, np.float32).ravel()
        emb = np.zeros(max(self.speaker_dim(), 1), np.float32)
        _check(_lib.q3t_speaker_encode(self.h, x, len(x), emb))
        return emb

    def encode_speakers(self, clips, strict=True):
        """q3t_speaker_encode_batch: many 24 kHz clips of any lengths through shared launches.  Returns (emb [n][dim],
        ok [n] bool); row c is bit for bit encode_speaker(clips[c]).  A clip too short for the encoder (< 5 mel
        frames) gets a zeroed row and ok False; with strict it raises instead, naming the clip's index."""
        xs = [np.ascontiguousarray(c, np.float32).ravel() for c in clips]
        n = len(xs)
        emb = np.zeros((n, max(self.speaker_dim(), 1)), np.float32)
        ok = np.zeros(n, np.int32)
        if n:
            ptrs = (C.POINTER(C.c_float) * n)(*[x.ctypes.data_as(C.POINTER(C.c_float)) for x in xs])
            lens = np.array([len(x) for x in xs], np.int32)
            _check(_lib.q3t_speaker_encode_batch(self.h, ptrs, lens, n, emb, None if strict else _addr(ok)))
            if strict:
                ok[:] = 1
        return emb, ok.astype(bool)

    def speaker_mel(self, samples):
        """the speaker encoder's log-mel front end, [n_frames][128] (time-major)"""
        x = np.ascontiguousarray(samples, np.float32).ravel()
        nf = C.c_int32(0)
        _check(_lib.q3t_speaker_mel(self.h, x, len(x), None, 0, C.byref(nf)))
        mel = np.zeros((max(nf.value, 1), 128), np.float32)
        _check(_lib.q3t_speaker_mel(self.h, x, len(x), _addr(mel), nf.value, C.byref(nf)))
        return mel[:nf.value]

    # ---- stages
    def talker_forward(self, embd, pos):
        embd = np.ascontiguousarray(embd, np.float32).reshape(-1, self.cfg["hidden"])
        n = embd.shape[0]
        pos = np.ascontiguousarray(np.broadcast_to(np.asarray(pos, np.int32), (n,)))
        hid = np.zeros((n, self.cfg["hidden"]), np.float32)
        lg = np.zeros((n, self.cfg["codec_vocab"]), np.float32)
        _check(_lib.q3t_talker_forward(self.h, n, embd, pos, _addr(hid), _addr(lg)))
        return hid, lg

    def talker_prefill(self, embd, family_slots=0):
        """causal prefill from position 0: embd [n_utt][n_rows][H] -> (hidden [n_utt][n_rows][H], last-row logits
        [n_utt][V]); K/V rows [0, n_rows) of slots 0..n_utt-1 (TTSTransformer::forward_prefill)"""
        H = self.cfg["hidden"]
        embd = np.ascontiguousarray(embd, np.float32)
        if embd.ndim == 2:
            embd = embd[None]
        n_utt, n_rows = embd.shape[0], embd.shape[1]
        hid = np.zeros((n_utt, n_rows, H), np.float32)
        lg = np.zeros((n_utt, self.cfg["codec_vocab"]), np.float32)
        _check(_lib.q3t_talker_prefill(self.h, n_utt, n_rows, embd.reshape(-1), int(family_slots), _addr(hid), _addr(lg)))
        return hid, lg

    def talker_prefill_ragged(self, embd_list, family_slots=0):
        """the same over prompts of different lengths in one pass (q3t_talker_prefill_ragged): embd_list[u] is
        [n_rows_u][H] with 1 <= n_rows_u <= 10 -> (list of hidden [n_rows_u][H], last-row logits [n_utt][V])"""
        H = self.cfg["hidden"]
        rows = [np.ascontiguousarray(e, np.float32).reshape(-1, H) for e in embd_list]
        n_rows = np.array([r.shape[0] for r in rows], np.int32)
        packed = np.ascontiguousarray(np.concatenate(rows, axis=0)).reshape(-1)
        hid = np.zeros((int(n_rows.sum()), H), np.float32)
        lg = np.zeros((len(rows), self.cfg["codec_vocab"]), np.float32)
        _check(_lib.q3t_talker_prefill_ragged(self.h, len(rows), n_rows, packed, int(family_slots), _addr(hid), _addr(lg)))
        off = np.concatenate([[0], np.cumsum(n_rows)])
        return [hid[off[u]:off[u + 1]].copy() for u in range(len(rows))], lg

    def codepred_frame(self, hidden, cb0, temperature=0.0, top_k=50, seed=0, frame=0, want_logits=False):
        hidden = np.ascontiguousarray(hidden, np.float32).reshape(-1, self.cfg["hidden"])
        n = hidden.shape[0]
        cb0 = np.ascontiguousarray(np.broadcast_to(np.asarray(cb0, np.int32), (n,)))
        codes = np.zeros((n, 15), np.int32)
        lg = np.zeros((n, 15, self.cfg["cp_vocab"]), np.float32) if want_logits else None
        _check(_lib.q3t_codepred_frame(self.h, n, hidden, cb0, float(temperature), int(top_k), int(seed), int(frame),
                                       codes, _addr(lg)))
        return (codes, lg) if want_logits else codes

    def cb0_select(self, logits, seen, frame, n_tokens, **params):
        p = default_params(**params)
        logits = np.ascontiguousarray(logits, np.float32).reshape(-1, self.cfg["codec_vocab"])
        n = logits.shape[0]
        seen = np.ascontiguousarray(seen, np.uint8).reshape(n, -1)
        frame = np.ascontiguousarray(np.broadcast_to(np.asarray(frame, np.int32), (n,)))
        nt = np.ascontiguousarray(np.broadcast_to(np.asarray(n_tokens, np.int32), (n,)))
        out = np.zeros(n, np.int32)
        _check(_lib.q3t_cb0_select(self.h, n, logits, seen, frame, nt, C.byref(p), out))
        return out

    def project_text(self, toks):
        toks = np.ascontiguousarray(toks, np.int32)
        out = np.zeros((len(toks), self.cfg["hidden"]), np.float32)
        _check(_lib.q3t_project_text(self.h, len(toks), toks, out))
        return out

    def prefill_embd(self, toks, speaker=None, language_id=2050):
        toks = np.ascontiguousarray(toks, np.int32)
        H = self.cfg["hidden"]
        pre = np.zeros((10, H), np.float32)
        tr = np.zeros((max(1, len(toks) - 8), H), np.float32)
        pad = np.zeros(H, np.float32)
        pl, tl = C.c_int32(0), C.c_int32(0)
        sp = None if speaker is None else np.ascontiguousarray(speaker, np.float32)
        _check(_lib.q3t_prefill_embd(self.h, toks, len(toks), _addr(sp), int(language_id), pre, C.byref(pl), tr,
                                     C.byref(tl), pad))
        return pre[:pl.value], tr[:tl.value], pad
