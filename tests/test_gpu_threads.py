"""Handles are per thread, the library is shared: two host threads, each with its own detector and recogniser handle on the same
GPU (own streams, own post-processing pools), run the whole pipeline at the same time - a serving process with several request
threads, or one thread per GPU (include/ocr_amd.h: a handle is not thread-safe, different handles are independent).  Every
result must be bit-identical to the same work done alone: no shared scratch, no library-wide state, thread-local errors.  The same
holds for the reading chain behind classify (glyphs, strips, lines, columns, lexicon, language model, lattice, both CTC decoders)
and for the batched preprocessing: two jobs of different shapes alone, stage by stage in turn, and from two threads."""
import threading

import numpy as np
import pytest

import ocr_rs_amd  # noqa: F401
from ocr_rs_amd import capi
from ocr_rs_amd import weights as W
from tests.test_gpu_config4 import run_pipeline

pytestmark = pytest.mark.gpu


def _same(a, b):
    pa, la, sa, ca, ba = a
    pb, lb, sb, cb, bb = b
    return (np.array_equal(pa, pb) and la == lb and len(sa) == len(sb)
            and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(sa, sb)) and np.array_equal(ca, cb) and np.array_equal(ba, bb))


def test_two_threads_two_handle_pairs_same_gpu_bit_identical():
    det_w, rec_w = W.make_det_weights_text(), W.make_rec_weights(0)
    blob_d, blob_r = W.pack_blob(det_w), W.pack_blob(rec_w)
    pages = [W.synth_text_pages(100 + t, 6, 640, 640)[0] for t in range(2)]
    precisions = [capi.PRECISION_F32, capi.PRECISION_BF16]   # one thread in each precision: different kernels side by side
    # alone, one after the other
    alone = []
    for t in range(2):
        det, rec = capi.Detector(blob_d, 0, options="post_threads=2"), capi.Recognizer(blob_r, 0)
        alone.append(run_pipeline(det, rec, pages[t], precisions[t]))
        det.close()
        rec.close()
    # together
    results, errors = [None, None], []
    start = threading.Barrier(2)

    def work(t):
        try:
            det, rec = capi.Detector(blob_d, 0, options="post_threads=2"), capi.Recognizer(blob_r, 0)
            start.wait()
            for _ in range(4):
                got = run_pipeline(det, rec, pages[t], precisions[t])
                if results[t] is not None and not _same(results[t], got):
                    errors.append(f"thread {t}: results changed between rounds")
                results[t] = got
            # an error on this thread stays on this thread
            with pytest.raises(capi.OcrError):
                det.forward_host(np.zeros((1, 1, 33, 32), np.float32))
            det.close()
            rec.close()
        except Exception as e:   # noqa: BLE001
            errors.append(f"thread {t}: {e!r}")

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(2):
        assert _same(alone[t], results[t]), f"thread {t}: concurrent result differs from the same work done alone"


# ---------------------------------------------------------------- the reading chain: everything after classify
#
# glyph segmentation by both rules, masks, splitting, straight and curved strips, group_lines, group_columns, glyph_costs,
# lexicon_match, lm_decode, lattice_decode, lexicon_lattice_match, both CTC decoders and preprocess_batch: two jobs of different
# shapes (tests/reading_jobs.py), each alone, then stage by stage in turn on two handle sets, then from two threads.

def _columns(det, rec, lex, lm, job):
    from ocr_rs_amd import reading
    return reading.read_columns(det, rec, job["frames"], job["polys"], job["adj"], cc={}, mask=True, lexicon=lex, lm=lm)


def _lines(det, rec, lex, lm, job):
    from ocr_rs_amd import reading
    return reading.read_lines(det, rec, job["frames"], job["polys"], job["adj"], rectified=False, lattice={}, lm=lm, lattice_lexicon=lex)


def _curved(det, rec, lex, lm, job):
    from ocr_rs_amd import reading
    return reading.read_words_rectified(det, rec, job["frames"], job["polys"], job["adj"], cc={}, curved=True)


def _words(det, rec, lex, lm, job):
    from ocr_rs_amd import reading
    return reading.read_words(det, rec, job["frames"], job["polys"], job["adj"], cc=None)


def _ctc(det, rec, lex, lm, job):
    return [rec.ctc_greedy_decode(job["logits"], job["blank"]), rec.ctc_beam_decode(job["logits"], job["blank"], job["beam"])]


def _preprocess(det, rec, lex, lm, job):
    return det.preprocess_batch(job["images"], 64, 32, want_f32=True)


STAGES = [_columns, _lines, _curved, _words, _ctc, _preprocess]


def run_reading(det, rec, lex, lm, job):
    """everything the reading chain produces for one job, stage by stage: one nested structure"""
    return [stage(det, rec, lex, lm, job) for stage in STAGES]


def _differs(a, b, at="result"):
    """where two such structures differ, or None: numpy arrays by their bytes (f64 and f32 as integers), everything else with =="""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        if not (isinstance(a, np.ndarray) and isinstance(b, np.ndarray)) or a.dtype != b.dtype or a.shape != b.shape:
            return f"{at}: array type or shape"
        return None if np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes() else f"{at}: array bytes"
    if isinstance(a, (list, tuple)) or isinstance(b, (list, tuple)):
        if type(a) is not type(b) or len(a) != len(b):
            return f"{at}: sequence type or length"
        for i, (x, y) in enumerate(zip(a, b)):
            d = _differs(x, y, f"{at}[{i}]")
            if d:
                return d
        return None
    return None if type(a) is type(b) and a == b else f"{at}: {a!r} != {b!r}"


class _Handles:
    """a fresh Detector, Recognizer, Lexicon and CharLm for one job"""

    def __init__(self, job):
        self.det = capi.Detector(W.pack_blob(W.make_det_weights(0)), 0)
        self.rec = capi.Recognizer(W.pack_blob(W.make_rec_weights(0)), 0)
        self.lex = capi.Lexicon(self.rec, job["words"])
        self.lm = capi.CharLm(self.rec, job["table"])
        self.all = (self.det, self.rec, self.lex, self.lm)

    def close(self):
        self.lm.close()
        self.lex.close()
        self.rec.close()
        self.det.close()


_ALONE = {}


def _alone(k):
    """the reference result of job k: alone, on handles of its own, computed once"""
    if k not in _ALONE:
        from tests import reading_jobs
        job = reading_jobs.job(k)
        h = _Handles(job)
        try:
            _ALONE[k] = run_reading(*h.all, job)
        finally:
            h.close()
    return _ALONE[k]


def test_reading_chain_alone_is_not_vacuous():
    from ocr_rs_amd import reading
    from oracle import ctc_oracle as CT
    from tests import ctc_beam_oracle as CB
    from tests import preprocess_batch_oracle as PB
    from tests import reading_jobs
    from tests.test_ctc_beam import _check, lds_case
    for k in range(2):
        job = reading_jobs.job(k)
        cols, lines, curved, words, (greedy, beam), (gray, fr, adj) = _alone(k)
        assert _differs(_alone(k), _alone(k)) is None and _differs(cols, lines) is not None
        n_words = [len(p) for p in job["polys"]]
        assert [len(pg) for pg in curved] == n_words and [len(pg) for pg in words] == n_words
        for b, where in enumerate(job["where"]):
            if k == 0:   # as test_read_columns_on_a_two_column_page: the left column's rows top to bottom, then the right column's
                assert [[[where[int(i)] for i in ks] for _, ks, _ in block] for block in cols[b]] == \
                    [[[(col, r, i) for i in range(3)] for r in range(4)] for col in range(2)]
            else:        # as test_read_lines_on_a_tilted_page: the rows top to bottom, each left to right
                rows, per = max(r for r, _ in where) + 1, max(i for _, i in where) + 1
                assert [[where[int(i)] for i in ks] for _, ks, _ in lines[b]] == [[(r, i) for i in range(per)] for r in range(rows)]
            assert sorted(int(i) for block in cols[b] for _, ks, _ in block for i in ks) == list(range(n_words[b]))
            assert sorted(int(i) for _, ks, _ in lines[b] for i in ks) == list(range(n_words[b]))
            assert reading.page_text(cols[b], columns=True).strip() and reading.page_text(lines[b]).strip()
            assert any(wd[0] for wd in curved[b]) and any(wd[0] for wd in words[b])
        if k == 0:
            assert [len(pg) for pg in lines] == [4, 8]        # the line rule on the two-column pages: merged at 50 px, interleaved at 90 px
        # the decoders against their oracles, the large case exactly the one tests/test_ctc_beam.py runs
        x, blank, bw = job["logits"], job["blank"], job["beam"]
        want = lds_case("limits, few classes")[3] if k == 0 else CB.ctc_beam_decode(x, blank, bw)
        assert _check(beam, want, f"job {k}", exact_ties=False).all()
        wl, wn = CT.ctc_greedy_decode(x, blank)
        assert np.array_equal(greedy[0], wl) and np.array_equal(greedy[1], wn)
        # the frames against the preprocessing oracle
        og, oadj = PB.preprocess_batch(job["images"], 64, 32)
        assert np.array_equal(gray, og) and (adj == oadj).all()
        assert np.array_equal(fr[:, 0].view(np.uint32), og.astype(np.float32).view(np.uint32))
    assert _differs(_alone(0)[5], _alone(1)[5]) is not None


def test_reading_chain_in_turn_on_two_handle_sets_bit_identical():
    """one thread, both handle sets open at once, stage k of job 0 then stage k of job 1: deterministic, and it catches any cache or
    table the library keeps per process and not per handle"""
    from tests import reading_jobs
    jobs = [reading_jobs.job(k) for k in range(2)]
    want = [_alone(k) for k in range(2)]
    sets = []
    try:
        for k in range(2):
            sets.append(_Handles(jobs[k]))
        for rnd in range(2):
            for s, stage in enumerate(STAGES):
                for k in range(2):
                    d = _differs(stage(*sets[k].all, jobs[k]), want[k][s], f"round {rnd}, job {k}, {stage.__name__}")
                    assert d is None, d
    finally:
        for h in sets:
            h.close()


@pytest.mark.timeout(300)
def test_reading_chain_from_two_threads_bit_identical():
    from tests import reading_jobs
    jobs = [reading_jobs.job(k) for k in range(2)]
    want = [_alone(k) for k in range(2)]
    errors = [[], []]
    start = threading.Barrier(2)

    def work(t):
        h = None
        try:
            h = _Handles(jobs[t])
            start.wait(60)
            for rnd in range(3):
                d = _differs(run_reading(*h.all, jobs[t]), want[t], f"thread {t}, round {rnd}")
                if d:
                    errors[t].append(d)
            # a refused call on this thread raises on this thread
            try:
                h.rec.ctc_beam_decode(jobs[1]["logits"], 9, 33)
                errors[t].append(f"thread {t}: a beam width of 33 was not refused")
            except capi.OcrError as e:
                if e.code != 1:
                    errors[t].append(f"thread {t}: {e!r}")
        except Exception as e:   # noqa: BLE001
            start.abort()
            errors[t].append(f"thread {t}: {e!r}")
        finally:
            if h is not None:
                h.close()

    threads = [threading.Thread(target=work, args=(t,), daemon=True) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(240)
        assert not th.is_alive(), "a reading thread did not return"     # (nothing more is started after a failed join)
    assert errors == [[], []], errors


def test_destroy_with_async_work_on_the_callers_stream():
    """`ocr_det_set_stream` + `ocr_det_forward_async` / `ocr_rec_classify_async`, then destroy WITHOUT synchronising: the handle
    drains the caller's stream before it frees the workspace those launches use - the results are complete and correct."""
    import torch
    det_w, rec_w = W.make_det_weights(0), W.make_rec_weights(0)
    x = torch.from_numpy(W.synth_image_batch(3, 8, 320, 320)).cuda()
    crops = torch.from_numpy(W.synth_crops(4, 2000)).cuda()
    ref_det, ref_rec = capi.Detector(W.pack_blob(det_w), 0), capi.Recognizer(W.pack_blob(rec_w), 0)
    want = torch.empty_like(x)
    ref_det.forward_device(x.data_ptr(), 8, 320, 320, want.data_ptr())
    ref_det.synchronize()
    want_lab = torch.empty(2000, dtype=torch.int32, device="cuda")
    want_pr = torch.empty(2000, dtype=torch.float64, device="cuda")
    ref_rec.classify_device(crops.data_ptr(), 2000, 0, want_lab.data_ptr(), want_pr.data_ptr())
    ref_rec.synchronize()
    ref_det.close()
    ref_rec.close()
    stream = torch.cuda.Stream()
    for _ in range(3):
        det, rec = capi.Detector(W.pack_blob(det_w), 0), capi.Recognizer(W.pack_blob(rec_w), 0)
        det.set_stream(stream.cuda_stream)
        rec.set_stream(stream.cuda_stream)
        got = torch.zeros_like(x)
        lab = torch.zeros(2000, dtype=torch.int32, device="cuda")
        pr = torch.zeros(2000, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        for _ in range(3):   # a queue of work behind the handle's back
            det.forward_device(x.data_ptr(), 8, 320, 320, got.data_ptr())
            rec.classify_device(crops.data_ptr(), 2000, 0, lab.data_ptr(), pr.data_ptr())
        det.close()   # no synchronize
        rec.close()
        torch.cuda.synchronize()
        assert torch.equal(got, want) and torch.equal(lab, want_lab) and torch.equal(pr, want_pr)
