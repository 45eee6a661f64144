"""gmx_chainstep_byte: the arithmetic decoder and ModPPMD's range walk on the device, a whole byte per call
(include/gmxmix_decoder.h, gmx_coder.hip).  The yardstick is the existing per-bit path: gmx_chainstep_step driven by a
Python restatement of the reference's Decoder and of the walk (tests/decoder_common.py) on a second, identically built
chain.  Equal to it, exactly (floats as bit patterns): every byte, its eight p, the coder state after every byte, and
at the end -- after the closing learn-only step -- every bank's export and the context boards."""
import numpy as np
import pytest

import decoder_common as dc
from gmix_amd import GmxError

pytestmark = pytest.mark.gpu

GMX_ERR_INVALID, GMX_ERR_STATE = -1, -5
TEXT = b"the cat sat on the mat. "     # 24 bytes, repeated by the encoder's stream


def run(rig, inputs, n_bytes, ppm, by_bytes, check_counter=True):
    """n_bytes[s] bytes of every stream, all streams together while they last; the closing learn-only step."""
    st = dc.decode_streams(rig, inputs)
    before = rig.cs.bit_launches
    for k in range(max(n_bytes)):
        group = [s for s in range(rig.S) if k < n_bytes[s]]
        (dc.byte_round if by_bytes else dc.bits_round)(rig, st, group, ppm)
    if by_bytes and check_counter and len(set(n_bytes)) == 1:
        assert rig.cs.bit_launches == before      # no per-bit graph across the byte calls
    dc.learn_only(rig, st, range(rig.S))
    return st


def encoded_text(gpu, S, n_bytes, ppm):
    """The per-bit path's own encoding of a repetitive text: the chain codes the known bits, oracle.encode packs them
    under the p it answered; one byte in the middle is flipped afterwards (improbable bits, multi-byte shifts)."""
    from oracle import gmxo
    rig = dc.Rig(gpu, "small", S, decoder=False)
    text = (TEXT * (n_bytes // len(TEXT) + 1))[:n_bytes]
    st = [dc.Stream(dc.Known(text)) for _ in range(S)]
    for _ in range(n_bytes):
        dc.bits_round(rig, st, list(range(S)), ppm)
    dc.learn_only(rig, st, range(S))
    rig.close()
    src = st[1].src
    payload = bytearray(gmxo.encode(src.bits, np.array(src.p, np.float32)))
    payload[len(payload) // 2] ^= 0x5A
    return bytes(payload), text


def test_small_chain_three_inputs(gpu):
    """General mixers, context bank, Indirect and Match banks, no LSTM; S = 3, 24 bytes: 200 random bytes, the chain's
    own encoding of a text with a byte flipped in the middle, and a 5-byte input that runs dry."""
    S, NB = 3, 24
    ppm = dc.make_ppm(S, NB, 7)
    payload, text = encoded_text(gpu, S, NB, ppm)
    rng = np.random.default_rng(99)
    inputs = [bytes(rng.integers(0, 256, 200, dtype=np.uint8)), payload, b"\x9c\x31\x07\xee\x42"]
    a = dc.Rig(gpu, "small", S, decoder=False)
    st_a = run(a, inputs, [NB] * S, ppm, False)
    assert bytes(st_a[1].bytes[:4]) == text[:4]                     # up to the flip the text comes back
    assert bytes(st_a[1].bytes) != text
    assert st_a[2].states[-1][3] == 5 and st_a[0].states[-1][3] < 200  # the short input ran dry, the long one did not
    b = dc.Rig(gpu, "small", S)
    st_b = run(b, inputs, [NB] * S, ppm, True)
    dc.assert_same(st_a, st_b, a, b)
    a.close()
    b.close()


@pytest.mark.parametrize("path", ["host_stores", "device_fetch"])
def test_stock_shape_with_the_lstm(gpu, path, monkeypatch):
    """The reference's own shape with the LSTM byte model: S = 2, 105 bytes (a backward pass of the LSTM falls inside
    the byte calls); the LSTM's long and short sections join the exports."""
    if path == "device_fetch":
        monkeypatch.setenv("GMX_CS_NO_BAR", "1")
    S, NB = 2, 105
    ppm = dc.make_ppm(S, NB, 11)
    rng = np.random.default_rng(5)
    inputs = [bytes(rng.integers(0, 256, 300, dtype=np.uint8)), bytes(rng.integers(0, 256, 40, dtype=np.uint8))]
    a = dc.Rig(gpu, "stock", S, with_lstm=True, decoder=False)
    st_a = run(a, inputs, [NB] * S, ppm, False)
    b = dc.Rig(gpu, "stock", S, with_lstm=True)
    st_b = run(b, inputs, [NB] * S, ppm, True)
    dc.assert_same(st_a, st_b, a, b)
    a.close()
    b.close()


def ragged_inputs(S):
    rng = np.random.default_rng(41)
    return [bytes(rng.integers(0, 256, 120, dtype=np.uint8)) for _ in range(S)]


def positive_ppm(S, n, seed):
    """(No zero mass: a stream that changes between the paths takes ModPPMD's slot value of a silent bit along.)"""
    rng = np.random.default_rng(seed)
    ppm = rng.random((S, n, 256), dtype=np.float32) + np.float32(1e-3)
    ppm /= ppm.sum(axis=2, keepdims=True, dtype=np.float32)
    return ppm.astype(np.float32)


def test_ragged_participation(gpu):
    """Stream 0 stops after byte 5, stream 1 joins at byte 3 (in the yardstick they simply code 5 and 9 bytes: streams do
    not see each other), stream 2 alternates per-bit steps and byte calls, stream 3 takes every byte."""
    S, NB = 4, 12
    ppm = positive_ppm(S, NB, 13)
    inputs = ragged_inputs(S)
    n_bytes = [5, NB - 3, NB, NB]
    a = dc.Rig(gpu, "small", S, decoder=False)
    st_a = run(a, inputs, n_bytes, ppm, False)
    b = dc.Rig(gpu, "small", S)
    st_b = dc.decode_streams(b, inputs)
    for k in range(NB):
        takers = [s for s in (0, 1, 3) if (s != 0 or k < 5) and (s != 1 or k >= 3)]
        if k % 3 == 1:                        # stream 2: a byte of per-bit steps, the host decoding from the device's state
            dc.bits_round(b, st_b, [2], ppm)
        else:
            takers.append(2)
        dc.byte_round(b, st_b, sorted(takers), ppm)
    dc.learn_only(b, st_b, range(S))
    dc.assert_same(st_a, st_b, a, b)
    a.close()
    b.close()


def test_seventy_streams_two_tail_blocks(gpu):
    """gmx_coder_tail_kernel takes a lane per stream: S = 70 is a full block and one with six live lanes, and the answer
    area's parts (take | decoded | byte_p | state) lie at rounded offsets that S = 70 does not fill.  Three bytes.
    Streams 0 .. 3 have inputs of 0, 1, 2 and 3 bytes (the four start bytes already read past the end), streams 64 and
    69 -- the second block's first and last live lane -- 50 bytes, the others 20.  Streams 5 and 66 sit byte 1 out, one in
    each block (in the yardstick they simply code two bytes): nothing of theirs is written by that call.  (Whether the
    tail stamped them cannot be seen from here: this shape's wait is the stream's synchronisation, not the stamps'.)"""
    S, NB, OUT = 70, 3, (5, 66)
    ppm = dc.make_ppm(S, NB, 23)
    rng = np.random.default_rng(70)
    lens = [0, 1, 2, 3] + [20] * (S - 4)
    lens[64] = lens[69] = 50
    inputs = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in lens]
    a = dc.Rig(gpu, "small", S, decoder=False)
    st_a = run(a, inputs, [NB - 1 if s in OUT else NB for s in range(S)], ppm, False)
    assert [st_a[s].states[-1][3] for s in range(4)] == [0, 1, 2, 3]
    b = dc.Rig(gpu, "small", S)
    st_b = dc.decode_streams(b, inputs)
    for k in range(NB):
        group = [s for s in range(S) if k != 1 or s not in OUT]
        kept = {s: (int(b.cs.decoded[s]), b.cs.byte_p[s].tobytes(), b.cs.decoder_state(s)) for s in OUT}
        dc.byte_round(b, st_b, group, ppm)
        if k == 1:
            for s in OUT:
                assert (int(b.cs.decoded[s]), b.cs.byte_p[s].tobytes(), b.cs.decoder_state(s)) == kept[s], s
                assert kept[s] == (st_b[s].bytes[0], np.array(st_b[s].p[0], np.uint32).tobytes(), st_b[s].states[0]), s
    dc.learn_only(b, st_b, range(S))
    dc.assert_same(st_a, st_b, a, b)
    a.close()
    b.close()


@pytest.mark.parametrize("n_inputs, slot", [(None, 37), (72, 70)], ids=["second_mask_word", "second_row_trip"])
def test_ppmd_slot_position(gpu, n_inputs, slot):
    """gmx_coder_step_kernel writes the prediction row 64 slots a trip and the mask word of ModPPMD's slot.  Slot 37 of
    the 40 inputs: the slot's word is mask word 1.  Slot 70 of 72 inputs (n_pad = 72: the row takes two trips, the mask
    three words): the slot lies in the second trip and in word 2.  Six bytes of make_ppm; stream 1's input is all
    zeros, so x is 0, every bit decodes as 1, and its slot is active (bytes 0, 1, 3, 5), inactive (the uniform byte 2)
    and silent (byte 4 has no mass above 127, where the first 1 leads)."""
    S, NB = 2, 6
    ppm = dc.make_ppm(S, NB, 29)
    inputs = [ragged_inputs(1)[0], bytes(40)]
    rigs = [dc.Rig(gpu, "small", S, decoder=on, n_inputs=n_inputs, ppmd_slot=slot) for on in (False, True)]
    a, b = rigs
    assert a.ppmd_slot == slot and (a.cs.predictions.shape[1] > 64) == (slot >= 64) and slot >> 5 == a.cs.mask_words - 1
    st_a = run(a, inputs, [NB] * S, ppm, False)
    assert st_a[1].bytes == [255] * NB
    st_b = run(b, inputs, [NB] * S, ppm, True)
    dc.assert_same(st_a, st_b, a, b)
    a.close()
    b.close()


def test_resume_in_a_fresh_object_and_two_objects_in_halves(gpu):
    """Six bytes, then every bank moves through its group export / import into a fresh chain whose decoders resume from
    decoder_state, six more bytes: equal to twelve bytes in one go.  And two objects driven alternately in launch / wait
    halves answer what each answers alone."""
    S, NB = 2, 12
    ppm = positive_ppm(S, NB, 17)
    inputs = ragged_inputs(S)
    a = dc.Rig(gpu, "small", S, decoder=False)
    st_a = run(a, inputs, [NB] * S, ppm, False)
    b1 = dc.Rig(gpu, "small", S)
    st_b = dc.decode_streams(b1, inputs)
    for _ in range(6):
        dc.byte_round(b1, st_b, [0, 1], ppm)
    dc.learn_only(b1, st_b, range(S))
    states = [b1.cs.decoder_state(s) for s in range(S)]
    b1.cs.close()
    b2 = dc.Rig(gpu, "small", S)
    b2.mg.import_all(b1.mg.export_all())
    b2.ig.import_all(b1.ig.export_all())
    b2.xg.import_all(*b1.xg.export_all())
    data, off, _ = b1.cg.group_export()
    b2.cg.group_import(data, off)
    b2.cg.set_group_blackboards(b1.cg.group_blackboards())
    for s in range(S):
        b2.ig.set_slot_values(b1.ig.slot_values(s), s)
        v, nb = b1.xg.slot_values(s)
        b2.xg.set_slot_values(v, nb, s)
        b2.cs.set_input(s, inputs[s], states[s])
        st_b[s].on_device = True
    for _ in range(6):
        dc.byte_round(b2, st_b, [0, 1], ppm)
    dc.learn_only(b2, st_b, range(S))
    dc.assert_same(st_a, st_b, a, b2)
    b1.close()
    b2.close()
    # two objects, the halves interleaved: launch x, launch y, wait x, wait y
    x, y = dc.Rig(gpu, "small", S), dc.Rig(gpu, "small", S)
    st_x, st_y = dc.decode_streams(x, inputs), dc.decode_streams(y, inputs[::-1])
    ppm_y = ppm[::-1]
    for _ in range(4):
        dc.byte_begin(x, st_x, [0, 1], ppm, call=x.cs.byte_launch)
        dc.byte_begin(y, st_y, [0, 1], ppm_y, call=y.cs.byte_launch)
        x.cs.byte_wait()
        dc.byte_end(x, st_x, [0, 1])
        y.cs.byte_wait()
        dc.byte_end(y, st_y, [0, 1])
    for s in range(S):
        want = tuple(part[:4] for part in st_a[s].log())
        assert st_x[s].log() == want, s
        assert st_y[S - 1 - s].log() == want, s
    x.close()
    y.close()
    a.close()


def test_refusals(gpu):
    """Every refusal leaves the chain where it was: the three bytes around them are the yardstick's, bit for bit."""
    import goldenlib
    import test_gpu_chainstep_match as tm
    S, NB = 2, 3
    ppm = positive_ppm(S, NB, 19)
    inputs = ragged_inputs(S)
    a = dc.Rig(gpu, "small", S, decoder=False)
    st_a = run(a, inputs, [NB] * S, ppm, False)

    def refused(call, status):
        with pytest.raises(GmxError) as e:
            call()
        assert e.value.status == status

    # attach without a context bank; with an unowned column (Indirect column 3 stays the caller's)
    _, z = goldenlib.load("ind_tiny_dense")
    mg = gpu.MixerGroup(a.topo, S)
    ig = gpu.IndirectGroup(tm.IND_MODELS, z["ns_next"], z["rm_next"], S, slots=tm.IND_SLOTS)
    cg = gpu.CtxGroup(dc.cc.fixture("ctx_tiny").descs, S)
    plain = gpu.ChainStep(mg)
    refused(lambda: plain.attach_decoder(11), GMX_ERR_INVALID)
    plain.close()
    loose = gpu.ChainStep(mg, ig)
    loose.attach_ctx(cg, [3, 13, 0, 7, 14, 16], [0, 1, 2, -1, 4])
    refused(lambda: loose.attach_decoder(11), GMX_ERR_INVALID)
    loose.close()
    for h in (cg, ig, mg):
        h.close()
    # a device-written ppmd_slot, one outside the record; then the attach that holds
    c = dc.Rig(gpu, "small", S, decoder=False)
    for slot in (tm.MSLOTS[0], tm.IND_SLOTS[1][0], -1, 40):
        refused(lambda: c.cs.attach_decoder(slot), GMX_ERR_INVALID)
    c.cs.attach_decoder(c.ppmd_slot)
    refused(lambda: c.cs.attach_decoder(c.ppmd_slot), GMX_ERR_STATE)
    c.cs.take[:] = [1, 0]
    refused(c.cs.byte, GMX_ERR_STATE)             # no input yet
    st_c = dc.decode_streams(c, inputs)
    c.cs.take[:] = [2, 1]
    refused(c.cs.byte, GMX_ERR_INVALID)
    dc.byte_round(c, st_c, [0, 1], ppm)           # byte 0
    c.cs.take[:] = [1, 0]
    refused(c.cs.byte, GMX_ERR_STATE)             # stream 1's Learn is outstanding: it may not sit the byte out
    calls = [0]

    def step_with_refusals():
        calls[0] += 1
        if calls[0] in (2, 5, 8):                 # inside byte 1, which goes through per-bit steps
            c.cs.take[:] = 1
            refused(c.cs.byte, GMX_ERR_STATE)     # a byte call inside a byte
            c.cs.launch()
            refused(c.cs.byte_launch, GMX_ERR_STATE)                  # between launch and wait
            refused(lambda: c.cs.set_input(0, inputs[0]), GMX_ERR_STATE)
            c.cs.wait()
        else:
            c.cs.step()
    dc.bits_round(c, st_c, [0, 1], ppm, step=step_with_refusals)      # byte 1
    dc.byte_begin(c, st_c, [0, 1], ppm, call=c.cs.byte_launch)        # byte 2
    refused(c.cs.byte_launch, GMX_ERR_STATE)      # between launch and wait
    refused(c.cs.launch, GMX_ERR_STATE)
    c.cs.byte_wait()
    dc.byte_end(c, st_c, [0, 1])
    dc.learn_only(c, st_c, range(S))
    dc.assert_same(st_a, st_c, a, c)
    # a byte call after a bank was destroyed
    c.xg.close()
    c.xg = None
    c.cs.take[:] = 1
    refused(c.cs.byte, GMX_ERR_STATE)
    c.close()
    a.close()
