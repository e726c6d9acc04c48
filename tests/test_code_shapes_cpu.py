"""The shapes of tests/code_shapes.py without a GPU: every shape builds and has the property it was chosen for, its encoder and its
codewords are right, its batches meet the conditions the GPU tests rely on, the scalar oracle and the CPU port agree on it, and the
host forms of the library - the definitions the device calls of tests/test_gpu_code_shapes.py are held to - equal their numpy
restatements on it."""
import numpy as np
import pytest

import code_shapes as cs
import early_stop_ref as esr
import encode_line_ref as el
import encoder_ref as er
import fec_status_ref as fs
import line_capture_ref as lc
import line_ref as lr

SHAPES = pytest.mark.parametrize("name", cs.NAMES)


@SHAPES
def test_shape_builds_and_has_its_property(abi, lib, name):
    shape = cs.describe(name)
    cs.check_structure(shape)
    assert shape == cs.describe(name)  # deterministic
    p = cs.properties(shape, abi, lib)
    print(name, "degrees", p["degrees"], "column weights", sorted(set(p["column_weights"].tolist())), "weight-3 columns", p["n_wcols"],
          "per layer", p["w_per_layer"], "bfw_fits", p["bfw_fits"], "zero-shift groups", p["zero_groups"], "LDS bytes", p["lds_bytes"])
    cs.check_properties(name, p)
    h = cs.code(name)
    # the degree classes are the runs of equal degree
    runs = [d for i, d in enumerate(p["degrees"]) if i == 0 or d != p["degrees"][i - 1]]
    assert list(h.deg) == runs and sum(h.deg_rows) == h.M and h.code.n_edges == 256 * sum(p["degrees"])
    assert p["lds_bytes"] <= 0xffff and (h.N - shape.puncture_tail) % 32 == 0


def test_the_table_spans_what_it_claims():
    tails = {cs.describe(n).puncture_tail for n in cs.NAMES}
    assert 0 in tails and any(t % 256 for t in tails) and any(t and t % 256 == 0 for t in tails)
    assert set(cs.BATCHES) == {(n, m) for n in cs.NAMES for m in cs.METHODS}


@SHAPES
def test_encoder_inverts_the_parity_part_and_codewords_satisfy_h(name):
    h, enc = cs.code(name), cs.encoder(name)
    H = er.parity_matrix(h)
    B = H[:, h.K:].astype(np.float32)
    v = np.random.default_rng(5).integers(0, 2, (h.M, 8)).astype(np.float32)
    back = np.rint(B @ (np.rint(enc.Binv.astype(np.float32) @ v) % 2)) % 2  # B (B^-1 v): float32 products below 2^24 are exact
    assert np.array_equal(back, v)
    # lower block-bidiagonal: nothing above the block diagonal
    assert not np.triu(H[:, h.K:].reshape(h.M // 256, 256, h.M // 256, 256).any(axis=(1, 3)), 1).any()
    cw = cs.batch(name, 2, "mixed")[1]
    assert cw[:, :h.K].any() and cw[:, h.K:].any()
    assert not esr.unsatisfied(h, cw).any()
    assert not fs.unsatisfied(h.code, cw).any()  # the second restatement, from the same pos_vn


@pytest.mark.parametrize("method", cs.METHODS)
@SHAPES
def test_batches_meet_their_conditions_and_the_oracle_equals_the_port(abi, lib, name, method):
    key = "m%d" % method
    (mixed, clean, scalar) = cs.references(abi, lib, [(name, key, "mixed"), (name, key, "clean"), (name, key, "mixed", "oracle")])
    h = cs.code(name)
    print(name, key, "mixed", mixed[1].tolist(), int(cs.wrong_frames(h, mixed[0], cs.batch(name, method, "mixed")[1]).sum()), "frames wrong; clean",
          clean[1].tolist())
    cs.check_batch_conditions(name, method, mixed, clean)
    assert np.array_equal(scalar[0], mixed[0]) and np.array_equal(scalar[1], mixed[1]), (scalar[1].tolist(), mixed[1].tolist())


@pytest.mark.parametrize("key", ["m0two", "m2ef1", "m2ef2", "m2classes", "m5classes"])
def test_variant_configurations_differ_from_their_base(abi, lib, key):
    """the variants the GPU tests add decode the mixed batch differently from the base configuration, so they test something"""
    name = "most" if key.endswith("classes") else "few"
    base, var = cs.references(abi, lib, [(name, key[:2], "mixed"), (name, key, "mixed")])
    assert not (np.array_equal(base[0], var[0]) and np.array_equal(base[1], var[1]))


@SHAPES
def test_encode_line_host_and_parity_inverse(abi, lib, name):
    h, enc = cs.code(name), cs.encoder(name)
    L = h.N - h.code.puncture_tail
    circ = abi.code_parity_inverse(h.code, lib)
    assert np.array_equal(er.unpack_parity_inverse(circ, h.M // 256), enc.Binv)
    n = 33
    payload, want_line, want_bits = el.expected(enc, el.messages(n, h.K, 300), L)
    line, bits = abi.encode_line_host(h.code, payload, n, True, lib, circ)
    assert np.array_equal(bits, want_bits) and np.array_equal(line, want_line)
    line1, none = abi.encode_line_host(h.code, payload[:1], 1, False, lib)
    assert np.array_equal(line1, want_line[:1]) and none is None


@SHAPES
def test_fec_status_host_forms(abi, lib, name):
    h = cs.code(name)
    fix, cw = cs.batch(name, 2, "mixed")
    out, st = cs.reference(abi, lib, name, "m2", "mixed")
    sent = cs.group_layout(cw, h.K)
    want = fs.status(h.code, fix, out, sent, cs.NG, with_sent=True)
    assert (want[0]["unsatisfied"] > 0).any() and (want[0]["unsatisfied"] == 0).any() and want[0]["corrected"].any()
    got = abi.fec_status_host(h.code, fix, out, sent, cs.NG, vs_sent=True, lib=lib)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1] and got[2] == want[2], (got[1], want[1], got[2], want[2])
    got = abi.fec_status_packed_host(h.code, abi.pack_llr4(fix, lib), fs.pack_decisions(out), sent, cs.NG, vs_sent=True, lib=lib)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1] and got[2] == want[2]
    # without the channel input and without sent frames
    want = fs.status(h.code, None, out, None, cs.NG)
    got = abi.fec_status_host(h.code, None, out, None, cs.NG, lib=lib)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1] and got[2] is None


@pytest.mark.parametrize("fmt,magnitude", [(lr.HARD, 4), (lr.LLR4, 0)], ids=["hard4", "llr4"])
@SHAPES
def test_line_formats_round_trip(abi, lib, name, fmt, magnitude):
    h = cs.code(name)
    N, K, L = h.N, h.K, h.N - h.code.puncture_tail
    fix = cs.batch(name, 2, "mixed")[0]
    frames = cs.frames_of(fix, N, K)
    for n in (1, 33, 65):
        line = abi.line_from_fixinput(h.code, fix, n, fmt, lib) if n > 64 else abi.line_from_fixinput(h.code, fix[:((n + 31) // 32) * 32 * N], n, fmt, lib)
        assert np.array_equal(line, lr.line_of(frames[:n], L, fmt))
        llr4 = abi.line_to_llr4(h.code, line, fmt, magnitude, n, lib)
        assert np.array_equal(llr4, lr.llr4_of_line(line, n, N, K, L, fmt, magnitude))
        if fmt == lr.LLR4 and n == 65:
            # the round trip: what was below L comes back, the punctured tail is erased
            back = cs.frames_of(lr.unpack_nibbles(llr4), N, K)[:n]
            assert np.array_equal(back[:, :L], frames[:n, :L]) and not back[:, L:].any()


@SHAPES
def test_line_capture_host(abi, lib, name):
    h = cs.code(name)
    n = 33
    idx, lines, bits, sent = cs.capture_case(abi, lib, name, n)
    for fmt in (lc.HARD, lc.LLR4):
        line = lines[fmt]
        for select in (1, 2, 3):
            want = lc.capture(h.code, line, fmt, bits, sent, n, 7, select, 0, 256)
            found, rec, sections = abi.line_capture_host(h.code, line, fmt, bits, sent, n, 7, select, 0, 256, lib)
            assert found == want[0] and np.array_equal(rec, want[1].astype(rec.dtype))
            assert np.array_equal(np.concatenate([sections[k] for k in ("line", "bits", "error", "syndrome")], axis=1), want[2])
        assert 0 < want[0] < n and (want[1]["channel_errors"] > 0).all()


@pytest.mark.parametrize("bad,good", list(cs.REFUSED.items()))
def test_limit_shapes_sit_on_either_side_of_the_limit(abi, lib, bad, good):
    """the codes tests/test_gpu_code_shapes.py expects lnsfaid_create to refuse are refused by the library's host-side table build
    (LNSFAID_E_CODE = -2), and the neighbour that differs in the one property is accepted"""
    with pytest.raises(ValueError, match=": -2$"):
        abi.code_zero_shift_order(cs.build(cs.limit_shape(bad), abi).code, lib)
    shape = cs.limit_shape(good)
    assert len(abi.code_zero_shift_order(cs.build(shape, abi).code, lib)[0]) == shape.nbr
    if bad == "lds_over":
        nbc = cs.first_lds_overflow(shape.nbr)
        assert cs.limit_shape(bad).nbc == nbc == shape.nbc + 1 <= 256
        assert cs.lds_bytes(nbc * 256, shape.nbr * 256) > 0xffff >= cs.lds_bytes(shape.nbc * 256, shape.nbr * 256)
    if bad == "weight17":
        assert (cs.column_weights(cs.limit_shape(bad)).max(), cs.column_weights(shape).max()) == (17, 16)


@pytest.mark.parametrize("name", list(cs.ROUND_TRIP_FLIPS))
def test_round_trip_channel_is_one_the_port_corrects(abi, lib, name):
    """encode_line -> binary symmetric channel -> decode_line of the GPU test: the CPU port under the per-codeword rule returns every
    sent codeword from the received line, so `corrected` must equal the flips there"""
    h = cs.code(name)
    n = 33
    payload, line, bits, thr, rx, flips = cs.round_trip_case(abi, lib, name, n)
    assert flips.sum() >= 10 and (flips == 0).any() and (flips >= 2).any(), flips.tolist()
    fix = lr.unpack_nibbles(abi.line_to_llr4(h.code, rx, abi.LINE_HARD, 4, n, lib))
    out, st = esr.per_codeword_oracle(h, cs.cfg_of(abi, lib, "m2"), fix, 2, kind="avx2", cws=list(range(n)))
    assert np.array_equal(fs.pack_decisions(out.reshape(-1)).reshape(n, -1), bits)
    assert (st[:, 0] < cs.MAX_ITER).all()
