"""Regenerates tests/golden/lstm_shapes.npz from the reference's own Lstm class at shapes other than the one LstmModel
builds (build container only: it needs the reference's sources and g++).  ref_lstm_shape_harness.cpp is compiled
against the reference's sources where they lie, into a temporary directory; the fixture holds the shape, the seeds, every
byte's distribution as uint32 and sha256 of the final gate weights, output layer and `.long` / `.short` bytes -- no
weights (the initial ones are re-drawn from the seed) and nothing of the reference's program text.

    python tests/golden/make_lstm_shape_golden.py [--ref /path/to/reference]

While generating, tests/lstm_shape_ref.c runs beside the reference: it must give the same bits, and its counters say
how often each of the three ClipGradients calls moved an element and how many backward passes ran.  The low-clip case
must clip at least once in state_error_ and in stored_error_; were that not so for its seed, another seed is chosen
HERE (synth seed 13 was, after 6 did not clip).  The third call, ClipGradients(hidden_error), can never move an element
of a one-layer model: LstmLayer::BackwardPass sets *hidden_error = 0 before it and only `layer > 0` adds to it, so its
counter is recorded as the 0 it must be.  The `hot*` cases must reach exact-zero softmax outputs, silent bits and clips in
both arrays on the restatement, or the script stops.
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import gmxo  # noqa: E402
import lstm_shape_common as lsc  # noqa: E402

# name, (cells, horizon, learning_rate, gradient_clip), bytes, srand seed, synth seed, synth mask, synth family
CASES = [
    ("tiny", (3, 2, 0.03, 10.0), 9, 11, 5, 255, 0),
    ("lowclip", (65, 7, 0.01, 0.05), 30, 12, 13, 255, 1),
    ("stock", (50, 100, 0.03, 10.0), 330, 0xDEADBEEF, 7, 255, 0),
    ("wide", (130, 5, 0.05, 10.0), 17, 14, 8, 63, 0),
    # the hard regimes, reached through learning_rate and gradient_clip alone: softmax outputs exactly 0, silent bits,
    # predictions at the logit clamp, hundreds of clipped elements (lstm_shape_common.regime_evidence counts them)
    ("hot255", (255, 9, 30.0, 0.05), 46, 5, 77, 255, 1),
    ("hot7", (7, 33, 100.0, 0.001), 200, 5, 77, 255, 1),
]

TUS = ["models/lstm.cpp", "models/lstm-layer.cpp", "memory/long-term-memory.cpp", "memory/short-term-memory.cpp",
       "mixer/mixer.cpp", "mixer/sigmoid.cpp", "contexts/nonstationary.cpp", "contexts/run-map.cpp"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("GMX_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=HERE, help="directory the fixture is written to")
    a = ap.parse_args()
    gmxo.build()
    out = {}
    names = []
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "ref_lstm_shape_harness")
        src = os.path.join(a.ref, "src")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-w", "-include", "cstring", "-ffp-contract=off", "-I" + src,
                               "-o", exe, os.path.join(HERE, "ref_lstm_shape_harness.cpp")] +
                              [os.path.join(src, t) for t in TUS])
        for name, shape, n, seed, sseed, mask, family in CASES:
            ppm, data = gmxo.lstm_synth(n, seed=sseed, mask=mask, family=family)
            fin, pre = os.path.join(td, name + ".in"), os.path.join(td, name)
            with open(fin, "wb") as f:
                f.write(np.ascontiguousarray(ppm, "<f4").tobytes())
                f.write(np.ascontiguousarray(data, np.uint8).tobytes())
            subprocess.check_call([exe, str(shape[0]), str(shape[1]), repr(float(np.float32(shape[2]))),
                                   repr(float(np.float32(shape[3]))), str(seed), str(n), fin, pre])
            probs = np.fromfile(pre + ".probs", "<u4").reshape(n, 256)
            long_b = open(pre + ".long", "rb").read()
            short_b = open(pre + ".short", "rb").read()
            cells, horizon = shape[0], shape[1]
            n_out = horizon * 256 * (cells + 1) * 4
            # the restatement beside it: same bits, and the counters the reference does not keep
            r = lsc.Ref(shape, seed=seed)
            got = r.run(ppm, data, learn=True)
            assert np.array_equal(lsc.u32(got["probs"]), probs), name
            assert r.export_long() == long_b and r.export_short() == short_b, name
            clips, passes = r.clip_counts(), r.backward_passes()
            assert passes >= 3, (name, passes)
            if name == "lowclip":
                assert min(clips[:2]) >= 1, ("choose another seed", clips)
            assert clips[2] == 0, (name, clips)
            if name.startswith("hot"):   # a hot case that is not hot pins nothing: choose another shape or seed HERE
                ev = lsc.regime_evidence(r, got)
                assert ev["nan"] == 0, (name, ev)
                assert ev["zero_probs"] > 0 and ev["silent_bits"] > 0 and min(clips[:2]) >= 1, (name, ev)
            names.append(name)
            rec = dict(cells=np.int32(cells), horizon=np.int32(horizon), lr=np.float32(shape[2]), clip=np.float32(shape[3]),
                       seed=np.uint32(seed), synth_seed=np.uint32(sseed), mask=np.uint32(mask), family=np.uint32(family),
                       n_bytes=np.uint32(n), probs=probs, sha_weights=np.array(lsc.sha(long_b[n_out:])),
                       sha_output_layer=np.array(lsc.sha(long_b[:n_out])), sha_long=np.array(lsc.sha(long_b)),
                       sha_short=np.array(lsc.sha(short_b)), clips=np.array(clips, np.uint64),
                       backward_passes=np.uint32(passes))
            for k, v in rec.items():
                out[name + "_" + k] = v
            print(name, shape, "bytes", n, "backward passes", passes, "clips", clips, "long", len(long_b), "short", len(short_b))
    np.savez_compressed(os.path.join(a.out, "lstm_shapes.npz"), names=np.array(names), **out)


if __name__ == "__main__":
    main()
