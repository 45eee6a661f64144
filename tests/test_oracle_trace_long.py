"""Whole-pipeline pins at length (VERDICT r1 #8a): they need the reference binaries of
oracle/_ref and the first 30 000 bytes of the reference's dictionary/english.dic, stored as
tests/golden/english_dic_30000.bin.

  * our strict build of the reference's CLI reproduces the survey's known answer: the first 30 000
    bytes of english.dic compress to 10 926 bytes, md5 abdf3dca43d06d93a6401515aa951167;
  * the oracle (oracle/gmx_oracle.c) replays all 240 000 bits of the reference Predictor's mixer
    boundary -- every one of the 33 outputs of every bit, the probability, the final state bytes --
    and its arithmetic coder restatement turns the probabilities into exactly that file's payload
    (5-byte length header in front, runner-utils.cpp:22-36);
  * the same with analysis on (predictions zeroed before every bit, predictor.cpp:362-365)."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from gmix_amd.bank import Topology
from trace_common import REF_TRACE, ROOT, make_trace

DIC = os.path.join(ROOT, "tests", "golden", "english_dic_30000.bin")   # english.dic[:30000]
GMIX = os.path.join(ROOT, "oracle", "_ref", "gmix_strict")
N = 30000

pytestmark = [pytest.mark.slow,
              pytest.mark.skipif(not (os.path.exists(DIC) and os.path.exists(REF_TRACE) and os.path.exists(GMIX)),
                                 reason="needs oracle/_ref (built where the reference's sources are)")]


@pytest.fixture(scope="module")
def compressed(tmp_path_factory):
    td = tmp_path_factory.mktemp("gmix")
    src = td / "in"
    src.write_bytes(open(DIC, "rb").read()[:N])
    subprocess.run([GMIX, "-c", str(src), str(td / "out")], check=True, cwd=td, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL, timeout=900)
    return (td / "out").read_bytes()


def test_strict_build_reproduces_the_surveys_known_answer(compressed):
    assert len(compressed) == 10926
    assert hashlib.md5(compressed).hexdigest() == "abdf3dca43d06d93a6401515aa951167"


@pytest.mark.parametrize("analysis", [0, 1])
def test_oracle_replays_240000_bits_of_the_reference_predictor(oracle, compressed, tmp_path, analysis):
    tr = make_trace(DIC, N, str(tmp_path / "t.bin"), analysis)
    assert tr["T"] == 8 * N and tr["n"] == 90 and tr["M"] == 33
    topo = Topology(tr["n"], tr["mixers"], tr["skip"])
    assert topo.weight_sizes() == tr["weight_sizes"]
    ob = oracle.Bank(tr["n"], topo.skip, topo.mixers)
    p, outs = ob.run(tr["pred"], tr["act"], tr["ctx"], tr["bits"])
    assert np.array_equal(outs.view(np.uint32), tr["outs"].view(np.uint32))
    assert np.array_equal(p.view(np.uint32), tr["p"].view(np.uint32))
    assert ob.export_long() == tr["long"] and ob.export_short() == tr["short"]
    # analysis on or off, the coded file is the same (tester.cpp:330-338 relies on it)
    payload = oracle.encode(tr["bits"], p)
    assert compressed[:5] == N.to_bytes(5, "big") and payload == compressed[5:]
