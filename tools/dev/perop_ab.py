"""dev: dump what the launch-per-op paths compute (every persistent kernel off), to compare two library variants bit
for bit: Q3T_DEV_LIB=<name> picks the library, every array a case returns is stored under "<case>.<index>".
Usage: perop_ab.py OUT.npz [CASE_PREFIX]   (CASE_PREFIX: only the cases whose name starts with it)
The cases: generate() on the vector stacks (2, 3 slots, and 3 slots with fused / deferred selection or the fused
code-predictor attention off), on the matrix-core stacks (4, 17, 70 slots; split attention; no layer-0 table; the
prefetch / gate-up tile knobs), the small and the 1.7B-layout models, talker_forward over positions crossing two
attention chunk edges, codepred_frame with its logits copies, the causal prefill per kernel family, and
generate_queue.  Each generate case runs 6 frames, once greedy and once sampled.
A library that reads Q3T_MM_PREFETCH / Q3T_MM_GU_TT when it is loaded only sees them in a process started with them:
run the "mm17_knobs" case again in such a process to compare it."""
import os
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(R, "qwen3-tts-jetson_amd"), os.path.join(R, "tests")]
os.environ.update(Q3T_PERSIST="0", Q3T_PERSIST_CP="0", Q3T_PERSIST_CPB="0", Q3T_PERSIST_TKB="0")
import q3t  # noqa: E402
from q3t_testutil import prompt, synth_dir  # noqa: E402

NF = 6
SAMPLING = (dict(temperature=0.0), dict(temperature=0.9, top_k=50, seed=77))
only = sys.argv[2] if len(sys.argv) > 2 else ""
out = {}


def engine(cfg, slots, max_ctx=96, **env):
    """a context created with `env` set: the options are read per context"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return q3t.Engine(synth_dir(cfg)[0], None, device=0, max_slots=slots, max_ctx=max_ctx)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def prompts(cfg, n):
    base = prompt(cfg)
    return [base[:4] + [(t + 13 * i) % 900 + 20 for t in base[4:]][:5 + i % 8] for i in range(n)]


def case(name, make, run):
    if not name.startswith(only):
        return
    eng = make()
    try:
        arrays = run(eng)
    finally:
        eng.close()
    for i, a in enumerate(arrays):
        out[f"{name}.{i}"] = np.asarray(a)
    print(name, len(arrays), "arrays", flush=True)


def gen(cfg, counts, queue_slots=0):
    def run(eng):
        res = []
        for n in counts:
            spk = [np.zeros(eng.cfg["hidden"], np.float32)] * n
            for kw in SAMPLING:
                if queue_slots:
                    res += eng.generate_queue(prompts(cfg, n), speakers=spk, max_len=NF, **kw)
                else:
                    res += eng.generate(prompts(cfg, n), speakers=spk, max_len=NF, force_frames=NF, **kw)
        return res
    return run


def talker_steps(eng):
    rng = np.random.default_rng(5)
    res = []
    for step in range(40, 140, 7):   # chunk edges at 64 and 128
        pos = (step + np.arange(32) % 13).astype(np.int32)
        res += eng.talker_forward((rng.standard_normal((32, eng.cfg["hidden"])) * 0.5).astype(np.float32), pos)
    return res


def cp_frames(eng):
    rng = np.random.default_rng(6)
    res = []
    for n in (1, 4):
        hid = (rng.standard_normal((n, eng.cfg["hidden"])) * 0.5).astype(np.float32)
        for kw in SAMPLING:
            res += eng.codepred_frame(hid, np.arange(n) * 37 + 5, frame=3, want_logits=True, **kw)
    return res


def prefills(eng):
    rng = np.random.default_rng(7)
    x = (rng.standard_normal((3, 10, eng.cfg["hidden"])) * 0.5).astype(np.float32)
    res = []
    for fam in (1, 4, 16):
        res += eng.talker_prefill(x, family_slots=fam)
    return res


case("vec_2_3", lambda: engine("full", 3), gen("full", (2, 3)))
for knob in ("Q3T_FUSED_SELECT", "Q3T_CP_DEFER_SELECT", "Q3T_CP_FUSED_ATTN"):
    case("vec3_" + knob, lambda: engine("full", 3, **{knob: "0"}), gen("full", (3,)))
case("mm_4_17_70", lambda: engine("full", 70), gen("full", (4, 17, 70)))
case("mm17_attn_split", lambda: engine("full", 17, Q3T_ATTN_SPLIT="1"), gen("full", (17,)))
case("mm4_no_cp_table", lambda: engine("full", 4, Q3T_MM_CP_TABLE="0"), gen("full", (4,)))
case("mm17_knobs", lambda: engine("full", 17, Q3T_MM_PREFETCH="2", Q3T_MM_GU_TT="1"), gen("full", (17,)))
case("tiny_1_4", lambda: engine("tiny", 4), gen("tiny", (1, 4)))
case("tiny17_1_4", lambda: engine("tiny17", 4), gen("tiny17", (1, 4)))
case("talker_forward32", lambda: engine("full", 32, max_ctx=160), talker_steps)
case("codepred_logits", lambda: engine("full", 4), cp_frames)
case("prefill_families", lambda: engine("full", 16), prefills)
case("queue_7_in_3", lambda: engine("full", 3), gen("full", (7,), queue_slots=3))
case("queue_14_in_6", lambda: engine("full", 6), gen("full", (14,), queue_slots=6))
np.savez(sys.argv[1], **out)
print("saved", len(out), "arrays")
