"""CTC greedy decode - an EXTENSION without a reference counterpart (the stage BASELINE.json's north_star / configs[2] name; the reference's
recogniser classifies single glyphs, /root/reference/src/char_recognition/model.rs:27-39).  The oracle (oracle/ctc_oracle.py, exact
integers) is pinned by hand-written vectors; the kernel (ocr-rs_amd/csrc/ctc.hip, one wave per crop) is held to the oracle bit for bit
through the C ABI at BASELINE configs[2]'s shape - N = 256 crops, T = 32 columns (a 32 x 128 crop at stride 4), C = 63 classes (the
alphabet of /root/reference/src/utils.rs:7-9 plus the blank) - and at the edges: all-blank crops, all-equal columns, tie columns, T = 1,
T beyond one wave's 64 columns, either end of the class range as the blank.  The second half of the file takes the kernel to its own
edges (chunk seams with placed classes, class counts up to 6625, blank positions, ragged workgroups, +-inf, the promise for a crop with
a NaN, refused calls, a caller-set stream), in host and device memory with guard rows around the outputs."""
import numpy as np
import pytest

from oracle import ctc_oracle as CT


def _onehot(seq, c, blank_fill=0.0):
    x = np.full((1, len(seq), c), blank_fill, np.float32)
    for t, k in enumerate(seq):
        x[0, t, k] = 1.0
    return x


def test_oracle_hand_vectors():
    B = 0
    lab, ln = CT.ctc_greedy_decode(_onehot([B, 3, 3, B, 3, 5, 5, 5, B, B, 7], 9), B)
    assert ln.tolist() == [4] and lab[0, :4].tolist() == [3, 3, 5, 7] and (lab[0, 4:] == -1).all()     # "a a _ a" keeps both a's
    lab, ln = CT.ctc_greedy_decode(_onehot([2, 2, 2, 2], 4), 0)
    assert ln.tolist() == [1] and lab[0, 0] == 2
    lab, ln = CT.ctc_greedy_decode(_onehot([3, 3, 3], 4), 3)                                             # all blank (blank = last class)
    assert ln.tolist() == [0] and (lab == -1).all()
    lab, ln = CT.ctc_greedy_decode(np.zeros((1, 5, 6), np.float32), 5)                                    # all-equal columns: class 0 wins every tie
    assert ln.tolist() == [1] and lab[0, 0] == 0
    lab, ln = CT.ctc_greedy_decode(np.zeros((1, 5, 6), np.float32), 0)                                    # ... which is the blank here
    assert ln.tolist() == [0]
    x = np.zeros((1, 3, 5), np.float32)
    x[0, 0, [2, 4]] = 1.0
    x[0, 1, [4, 2]] = 1.0
    x[0, 2, 1] = -0.0                                                                                     # -0.0 == 0.0: class 0 is first
    lab, ln = CT.ctc_greedy_decode(x, 0)
    assert ln.tolist() == [1] and lab[0, 0] == 2                                                          # ties: the lowest class, twice -> one label


def _cases():
    rng = np.random.default_rng(63)
    out = []
    x = rng.standard_normal((256, 32, 63)).astype(np.float32)                                 # BASELINE configs[2]'s shape
    x[:, :, 62] += 1.5                                                                        # a blank-heavy head, as trained CTC heads are
    x[3] = 0.0                                                                                # all-equal columns
    x[4, :, 62] = 9.0                                                                         # all blank
    x[5, :, :] = -1.0; x[5, :, 17] = 2.0                                                      # one class throughout
    x[6] = -1.0; x[6, ::2, 10] = 5.0; x[6, 1::2, 62] = 5.0                                                 # the same class between blanks: 16 labels
    x[7] = -1.0; x[7, :, 20] = 4.0; x[7, :, 40] = 4.0                                                      # a tie in every column
    out.append(("256x32x63", x, 62))
    out.append(("blank 0", rng.standard_normal((100, 32, 63)).astype(np.float32), 0))
    out.append(("T=1", rng.standard_normal((70, 1, 63)).astype(np.float32), 62))
    out.append(("T=200: chunks of 64 with a carried class", np.repeat(rng.standard_normal((9, 50, 11)).astype(np.float32), 4, axis=1), 10))
    out.append(("T=65", np.repeat(rng.standard_normal((5, 13, 7)).astype(np.float32), 5, axis=1), 3))
    out.append(("C=1: only the blank", np.zeros((3, 8, 1), np.float32), 0))
    out.append(("one crop", rng.standard_normal((1, 32, 63)).astype(np.float32), 31))
    return out


@pytest.mark.gpu
def test_device_ctc_greedy_decode_equals_the_oracle():
    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi
    from ocr_rs_amd import weights as W
    rec = capi.Recognizer(W.pack_blob(W.make_rec_weights(0)), 0)
    for name, x, blank in _cases():
        want_l, want_n = CT.ctc_greedy_decode(x, blank)
        got_l, got_n = rec.ctc_greedy_decode(x, blank)
        assert np.array_equal(got_n, want_n), name
        assert np.array_equal(got_l, want_l), name
    # device memory
    import torch
    name, x, blank = _cases()[0]
    xd = torch.from_numpy(x).cuda()
    lab = torch.empty((x.shape[0], x.shape[1]), dtype=torch.int32, device="cuda")
    ln = torch.empty(x.shape[0], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rec.ctc_greedy_decode_device(xd.data_ptr(), x.shape[0], x.shape[1], x.shape[2], blank, lab.data_ptr(), ln.data_ptr())
    want_l, want_n = CT.ctc_greedy_decode(x, blank)
    assert np.array_equal(lab.cpu().numpy(), want_l) and np.array_equal(ln.cpu().numpy(), want_n)
    assert int(want_n[6]) == 16 and int(want_n[4]) == 0 and int(want_n[3]) == 1 and int(want_n[7]) == 1
    with pytest.raises(capi.OcrError):
        rec.ctc_greedy_decode(x, 63)
    rec.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# The kernel at its edges: the seams between its 64-column chunks, class counts, blank positions, ragged workgroups, infinities, NaN,
# refused calls.  The cases are built (and their expectations checked against the oracle) on the CPU; the GPU tests hold the kernel to
# the oracle bit for bit in host and in device memory, each time into rows 1..N of outputs that carry a guard row of SENT either side.
SENT = -0x21524111     # 0xDEADBEEF as int32: never a class, a length or the -1 padding
SEAM_T = (63, 64, 65, 127, 128, 129, 192)
SEAMS = (63, 127)      # a seam lies between columns s and s + 1
PLACEMENTS = ("same", "different", "a blank a")


def _peaked(paths, c):
    """N x T classes -> logits N x T x C whose column maxima are those classes (noise well below the peak)"""
    paths = np.asarray(paths)
    x = np.random.default_rng(paths.size + c).uniform(-1.0, 1.0, size=paths.shape + (c,)).astype(np.float32)
    np.put_along_axis(x, paths[..., None], 4.0, axis=2)
    return x


def _seam_case(t, placement, blank, c=11):
    """(logits 5 x T x C, the length crop 0 must decode to).  Crop 0: every column another non-blank class than its neighbour, so all T
    are kept, then the placement at each seam; crop 1: runs of three columns (they straddle the seams); crop 2: one class throughout
    (one label, carried over every seam); crop 3: all blank (kept = 0: the whole row is padding); crop 4: a run that ENDS on the last
    column before each seam, and another class behind it."""
    nb = [k for k in range(c) if k != blank]
    a, b = nb[6], nb[7]
    p0 = [nb[i % 5] for i in range(t)]
    want = t
    for s in SEAMS:
        if placement == "same" and s < t:
            p0[s] = a
            if s + 1 < t:
                p0[s + 1] = a
                want -= 1                       # a a across the seam: one label
        elif placement == "different" and s < t:
            p0[s] = a
            if s + 1 < t:
                p0[s + 1] = b
        elif placement == "a blank a" and s < t:
            p0[s - 1], p0[s] = a, blank
            want -= 1                           # the blank is dropped ...
            if s + 1 < t:
                p0[s + 1] = a                   # ... and both a's stay
    rng = np.random.default_rng(t)
    p1 = np.repeat(rng.integers(0, c, size=t // 3 + 1), 3)[1:t + 1]
    p4 = [nb[1] if i % 64 in (61, 62, 63) else nb[2 + (i % 3)] for i in range(t)]
    return _peaked([p0, p1, [a] * t, [blank] * t, p4], c), want


def _blanks(c):
    return sorted({0, c // 2, c - 1})


def _well_formed(labels, lengths, c, blank):
    """every row: lengths[i] in [0, T], that many non-blank classes of [0, C), then -1"""
    n, t = labels.shape
    for i in range(n):
        k = int(lengths[i])
        assert 0 <= k <= t, (i, k)
        assert ((labels[i, :k] >= 0) & (labels[i, :k] < c) & (labels[i, :k] != blank)).all() and (labels[i, k:] == -1).all(), i


def test_seam_cases_decode_as_placed():
    for t in SEAM_T:
        for placement in PLACEMENTS:
            for blank in _blanks(11):
                x, want = _seam_case(t, placement, blank)
                lab, ln = CT.ctc_greedy_decode(x, blank)
                assert ln[0] == want and ln[2] == 1 and ln[3] == 0, (t, placement, blank, ln)
                _well_formed(lab, ln, 11, blank)
    # by hand at T = 65, blank 0 (non-blank classes 1..10, a = 7, b = 8): what stands around the seam 63 | 64
    ends = {}
    for placement in PLACEMENTS:
        x, want = _seam_case(65, placement, 0)
        lab, ln = CT.ctc_greedy_decode(x, 0)
        ends[placement] = lab[0, ln[0] - 3:ln[0]].tolist()
    assert ends == {"same": [2, 3, 7], "different": [3, 7, 8], "a blank a": [2, 7, 7]}
    x, _ = _seam_case(64, "a blank a", 0)      # T = 64: column 63 is the last, nothing follows the blank
    lab, ln = CT.ctc_greedy_decode(x, 0)
    assert ln[0] == 63 and lab[0, 62] == 7 and lab[0, 63] == -1


def _inf_case():
    inf = np.float32("inf")
    x = np.zeros((2, 4, 5), np.float32)
    x[:, 0, :] = -inf                                   # all -inf: class 0
    x[:, 1, :] = -1.0; x[:, 1, [2, 3]] = inf            # +inf twice: the lower class
    x[:, 2, :] = -inf; x[:, 2, 3] = -7.0                # one finite value among -inf
    x[:, 3, :] = 2.0; x[:, 3, 1] = inf
    x[1, 1, :] = -inf                                   # crop 1: two columns of -inf in a row -> class 0 once
    return x


def test_infinities_are_ordinary_values_in_the_oracle():
    lab, ln = CT.ctc_greedy_decode(_inf_case(), 4)
    assert ln.tolist() == [4, 3] and lab[0].tolist() == [0, 2, 3, 1] and lab[1].tolist() == [0, 3, 1, -1]
    lab, ln = CT.ctc_greedy_decode(_inf_case(), 0)      # ... and class 0 is the blank
    assert ln.tolist() == [3, 2] and lab[0].tolist() == [2, 3, 1, -1] and lab[1].tolist() == [3, 1, -1, -1]


def _edge_cases():
    """(name, logits, blank) beyond the seams: class counts, blank positions, ragged last workgroups (4 crops each)"""
    rng = np.random.default_rng(64)
    out = []
    for c, n, t in ((2, 5, 40), (64, 5, 20), (65, 5, 20), (6625, 5, 3)):
        x = rng.standard_normal((n, t, c)).astype(np.float32)
        x[0, 0, c - 1] = 9.0                            # the last class wins
        x[1, 0, :] = 0.5                                # a tie over the whole range: class 0
        x[2, 0, :] = -3.0; x[2, 0, [c // 2, c - 1]] = 8.0   # a tie of two: the lower
        x[3, :, 0] = 9.0                                # class 0 throughout
        x[4, :, c - 1] = 9.0                            # the last class throughout
        for blank in _blanks(c):
            out.append((f"C={c} blank={blank}", x, blank))
    for n in (1, 3, 4, 5, 257):
        x = np.repeat(rng.standard_normal((n, 11, 11)).astype(np.float32), 3, axis=1)    # T = 33, runs of three
        out.append((f"N={n}", x, 10))
    out.append(("largest", np.repeat(rng.standard_normal((257, 64, 11)).astype(np.float32), 3, axis=1), 5))      # 257 x 192 x 11
    for blank in (0, 4):
        out.append((f"infinities blank={blank}", _inf_case(), blank))
    return out


def _rec():
    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import capi
    from ocr_rs_amd import weights as W
    return capi.Recognizer(W.pack_blob(W.make_rec_weights(0)), 0)


def _raw(rec, logits_ptr, n, t, c, blank, mem_kind, labels_ptr, lengths_ptr):
    from ocr_rs_amd import capi
    return capi.lib().ocr_ctc_greedy_decode(rec._h, logits_ptr, n, t, c, blank, mem_kind, labels_ptr, lengths_ptr)


def _both_forms(rec, x, blank):
    """host and device memory, each into rows 1..N of (N + 2)-row outputs filled with SENT: asserts the guard rows and that the two
    forms agree, returns (labels N x T, lengths N)"""
    import torch
    from ocr_rs_amd import capi
    x = np.ascontiguousarray(x, np.float32)
    n, t, c = x.shape
    lab = np.full((n + 2, t), SENT, np.int32)
    ln = np.full(n + 2, SENT, np.int32)
    assert _raw(rec, x.ctypes.data, n, t, c, blank, capi.MEM_HOST, lab[1:].ctypes.data, ln[1:].ctypes.data) == 0
    xd = torch.from_numpy(x).cuda()
    dlab = torch.full((n + 2, t), SENT, dtype=torch.int32, device="cuda")
    dln = torch.full((n + 2,), SENT, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert _raw(rec, xd.data_ptr(), n, t, c, blank, capi.MEM_DEVICE, dlab.data_ptr() + 4 * t, dln.data_ptr() + 4) == 0
    dlab, dln = dlab.cpu().numpy(), dln.cpu().numpy()
    for a, b in ((lab, ln), (dlab, dln)):
        assert (a[0] == SENT).all() and (a[-1] == SENT).all() and b[0] == SENT and b[-1] == SENT     # exactly N x T labels, N lengths
    assert np.array_equal(lab, dlab) and np.array_equal(ln, dln)
    return lab[1:-1], ln[1:-1]


def _hold_to_oracle(rec, x, blank, tag):
    want_l, want_n = CT.ctc_greedy_decode(x, blank)
    got_l, got_n = _both_forms(rec, x, blank)
    assert np.array_equal(got_n, want_n), tag
    assert np.array_equal(got_l, want_l), tag
    _well_formed(got_l, got_n, x.shape[2], blank)


@pytest.mark.gpu
@pytest.mark.parametrize("t", SEAM_T)
def test_device_chunk_seams(t):
    rec = _rec()
    for placement in PLACEMENTS:
        for blank in _blanks(11):
            x, want = _seam_case(t, placement, blank)
            _hold_to_oracle(rec, x, blank, (t, placement, blank))
    rec.close()


@pytest.mark.gpu
def test_device_class_counts_blank_positions_crop_counts_infinities():
    rec = _rec()
    for name, x, blank in _edge_cases():
        _hold_to_oracle(rec, x, blank, name)
    rec.close()


@pytest.mark.gpu
def test_device_nan_crop_is_unspecified_but_well_formed():
    """the promise of include/ocr_amd.h for a crop that holds a NaN: the call succeeds, the row keeps its layout, the other crops of the
    batch equal the oracle"""
    rec = _rec()
    x = np.repeat(np.random.default_rng(65).standard_normal((6, 24, 9)).astype(np.float32), 3, axis=1)[:, :70]     # T = 70: two chunks
    clean = x.copy()
    x[2, 0, 0] = np.nan          # at the head of a column's scan
    x[2, 5, 4] = np.nan          # in its middle
    x[2, 63, :] = np.nan         # a whole column, the last of the first chunk
    x[2, 69, 8] = np.nan         # the last value of the crop
    for blank in (0, 4, 8):
        want_l, want_n = CT.ctc_greedy_decode(clean, blank)
        got_l, got_n = _both_forms(rec, x, blank)
        keep = [0, 1, 3, 4, 5]
        assert np.array_equal(got_n[keep], want_n[keep]) and np.array_equal(got_l[keep], want_l[keep]), blank
        _well_formed(got_l, got_n, 9, blank)
    rec.close()


@pytest.mark.gpu
def test_device_caller_set_stream():
    import torch
    rec = _rec()
    x, _ = _seam_case(129, "same", 5)
    st = torch.cuda.Stream()
    rec.set_stream(st.cuda_stream)
    _hold_to_oracle(rec, x, 5, "caller-set stream")
    rec.set_stream(None)
    _hold_to_oracle(rec, x, 5, "the handle's own stream again")
    rec.close()


@pytest.mark.gpu
def test_device_refused_calls_write_nothing_and_leave_the_handle_usable():
    import torch
    from ocr_rs_amd import capi
    rec = _rec()
    x, _ = _seam_case(65, "different", 10)
    n, t, c = x.shape
    lab = np.full((n, t), SENT, np.int32)
    ln = np.full(n, SENT, np.int32)
    xd = torch.from_numpy(x).cuda()
    dlab = torch.full((n, t), SENT, dtype=torch.int32, device="cuda")
    dln = torch.full((n,), SENT, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def call(*, r=rec, f=x.ctypes.data, n=n, t=t, c=c, blank=10, mk=capi.MEM_HOST, l=lab.ctypes.data, k=ln.ctypes.data):
        return capi.lib().ocr_ctc_greedy_decode(r._h if r is not None else None, f, n, t, c, blank, mk, l, k)

    dev = dict(f=xd.data_ptr(), l=dlab.data_ptr(), k=dln.data_ptr())
    refused = [dict(mk=2), dict(mk=7), dict(mk=-1), dict(mk=2, **dev), dict(mk=7, **dev),
               dict(r=None), dict(f=None), dict(l=None), dict(k=None),
               dict(t=0), dict(c=0), dict(c=0, blank=0), dict(blank=-1), dict(blank=c), dict(n=-1),
               dict(t=0, mk=capi.MEM_DEVICE, **dev), dict(blank=c, mk=capi.MEM_DEVICE, **dev), dict(n=-1, mk=capi.MEM_DEVICE, **dev)]
    for kw in refused:
        assert call(**kw) == 1, kw                    # OCR_ERR_INVALID
        assert capi.lib().ocr_last_error(), kw
        assert (lab == SENT).all() and (ln == SENT).all(), kw
        assert (dlab.cpu().numpy() == SENT).all() and (dln.cpu().numpy() == SENT).all(), kw
        _hold_to_oracle(rec, x, 10, ("after", kw))
    for kw in (dict(n=0), dict(n=0, mk=capi.MEM_DEVICE, **dev)):      # N = 0: success, nothing written
        assert call(**kw) == 0, kw
        assert (lab == SENT).all() and (ln == SENT).all() and (dlab.cpu().numpy() == SENT).all() and (dln.cpu().numpy() == SENT).all(), kw
    assert call() == 0
    want_l, want_n = CT.ctc_greedy_decode(x, 10)
    assert np.array_equal(lab, want_l) and np.array_equal(ln, want_n)
    rec.close()


@pytest.mark.gpu
def test_reference_named_mirror_decodes_to_strings():
    """char_recognition.Net.ctc_greedy_decode: classes 0..61 are the reference's alphabet (utils.rs:7), class 62 the blank"""
    import ocr_rs_amd  # noqa: F401
    from ocr_rs_amd import char_recognition as cr
    from ocr_rs_amd import weights as W
    net = cr.Net(W.pack_blob(W.make_rec_weights(0)), 0)
    word = [7, 7, 62, 30, 62, 37, 37, 62, 37, 40, 62, 62, 52, 53]        # H e l l o 0 1 with repeats and blanks
    x = np.full((2, len(word), 63), -4.0, np.float32)
    for t, k in enumerate(word):
        x[0, t, k] = 3.0
    x[1, :, 62] = 1.0                                                     # all blank
    assert net.ctc_greedy_decode(x) == ["Hello01", ""]
    net.close()
