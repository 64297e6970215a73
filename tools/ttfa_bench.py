"""Time to first audio: 0.4B synthetic model + full-dims synthetic vocoder, S = 512 semantic tokens.

Two cases, each measured in this process after a warm-up, from submit to PCM on the host:
  b1    one request alone: time to the first streamed chunk (stream_request, chunk_frames frames),
        and to the last one, against the time to the complete non-streamed PCM of the same request
        (generate + decode_audio);
  b32   the same for one streaming request beside 31 non-streaming ones (submitted just before it,
        decoding in the same engine; their vocoder pass is not part of either figure).
Usage: ttfa_bench.py [--out FILE.json] [--reps N] [--chunk FRAMES] [--S TOKENS]. Prints the JSON."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rwkv-tts-rs_amd"))
import numpy as np  # noqa: E402

import rwkvtts  # noqa: E402
from rwkvtts import codec as CC  # noqa: E402
from rwkvtts import weights as W  # noqa: E402
from rwkvtts.pipeline import LightweightTtsPipeline  # noqa: E402

PROPS = [77823, 77838, 77869, 77845, 77830, 77826]


def request(i, S):
    rs = np.random.RandomState(1000 + i)
    return rwkvtts.TtsBatchRequest(text_tokens=rs.randint(12293, 77822, size=24).tolist(), property_tokens=PROPS,
                                   args=rwkvtts.SamplerArgs(seed=i), fixed_semantic=S)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--S", type=int, default=512)
    a = ap.parse_args()
    blob = W.synth_blob(W.DIMS_04B, seed=20251205)
    mgr = rwkvtts.DynamicBatchManager(blob, config=rwkvtts.DynamicBatchConfig(max_batch_size=32, collect_timeout_ms=2),
                                      devices=[0], max_slots=32, token_chunk_size=512)
    del blob
    d = CC.CODEC_DIMS_FULL
    voc = CC.BiCodecDetokenizer(CC.synth_codec_blob(d), d)
    pipe = LightweightTtsPipeline(mgr, voc)
    H = voc.halo()

    def streamed(req):
        t0 = time.perf_counter()
        first = last = None
        n_chunks, h = 0, None
        parts = []
        for c in pipe.stream_request(req, a.chunk):
            last = time.perf_counter() - t0
            if first is None:
                first, h = last, c.n_known
            n_chunks += 1
            parts.append(np.asarray(c))
        return {"first_chunk_ms": first * 1e3, "last_chunk_ms": last * 1e3, "chunks": n_chunks,
                "tokens_known_at_first_chunk": h}, np.concatenate(parts)

    def plain(req):
        t0 = time.perf_counter()
        g, s = mgr.generate_tts_batch([req])[0]
        t_tok = time.perf_counter() - t0
        pcm = voc.decode_audio(g, s)
        return {"tokens_ms": t_tok * 1e3, "complete_pcm_ms": (time.perf_counter() - t0) * 1e3}, pcm

    def beside(fn, req, others):
        """fn(req) while `others` decode in the same engine (submitted first; waited for afterwards)."""
        tickets = [mgr.submit(r) for r in others]
        out = fn(req)
        for t in tickets:
            mgr.wait(t)
        return out

    def med(rows):
        return {k: round(statistics.median(r[k] for r in rows), 3) for k in rows[0]}

    res = {"model": "0.4B synthetic bf16", "codec": "full dims synthetic", "S": a.S, "chunk_frames": a.chunk,
           "halo_frames": H, "reps": a.reps, "build_id": rwkvtts._ffi.build_id()}
    for case, n_other in (("b1", 0), ("b32", 31)):
        others = [request(100 + i, a.S) for i in range(n_other)]
        req = request(7, a.S)
        beside(streamed, req, others)  # warm-up: graphs captured, buffers sized
        beside(plain, req, others)
        st, pl, same = [], [], True
        for _ in range(a.reps):
            s_row, s_pcm = beside(streamed, req, others)
            p_row, p_pcm = beside(plain, req, others)
            st.append(s_row)
            pl.append(p_row)
            same &= s_pcm.tobytes() == p_pcm.tobytes()
        res[case] = {"streamed": med(st), "non_streamed": med(pl), "streamed_all": st, "non_streamed_all": pl,
                     "pcm_bitwise_equal": bool(same)}
    mgr.close()
    voc.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
