"""Two reading jobs for tests/test_gpu_threads.py, chosen so that two handle sets that run them side by side never launch the same
shape: other pages (320 x 480 against 320 x 400, other word counts), a lexicon of one chunk pass against one of several, two
character models, CTC logits at the beam kernel's limits (T = 1024, B = 32, 97 KB of LDS) against its smallest use (T = 8, B = 2), and
other decoded images for the batched preprocessing.  Everything is seeded; a job is built once and never written to."""
import numpy as np

from tests import char_lm_oracle as CL
from tests import lexicon_oracle as LX

_JOBS = {}


def job(k: int) -> dict:
    if k not in _JOBS:
        _JOBS[k] = _build(k)
    return _JOBS[k]


def _build(k: int) -> dict:
    from tests.test_ctc_beam import lds_case
    from tests.test_gpu_columns import _two_column_frame
    from tests.test_gpu_lines import _tilted_page
    from tests.test_gpu_preprocess_batch import SIZES, images
    if k == 0:
        # the page of test_read_columns_on_a_two_column_page: 4 x 3 words a column, gutters of 50 and 90 px
        pages = [_two_column_frame(4, 3, 50.0, 0.1, 320, 480), _two_column_frame(4, 3, 90.0, -0.15, 320, 480)]
        x, blank, beam, _ = lds_case("limits, few classes")
        n_words, imgs = 300, images()[:4]
    else:
        # the pages of test_read_lines_on_a_tilted_page
        pages = [_tilted_page(4, 5, 0.25, 320, 400), _tilted_page(3, 4, -0.3, 320, 400)]
        x, blank, beam = np.random.default_rng(11).standard_normal((4, 8, 10)).astype(np.float32), 9, 2
        n_words, imgs = 5000, images()[len(SIZES) - 4:]
    rng = np.random.default_rng(900 + k)
    # entries of 1 .. 8 characters: a word of G glyphs meets the entries of G - 2 .. G + 2, about 5 / 8 of the list (one chunk pass of 256
    # entries for 300 words, a dozen for 5 000)
    words = LX.random_words(rng, n_words, 1, 8)
    table = CL.make_model(rng)
    assert np.count_nonzero(table) > 3000
    table.setflags(write=False)
    x.setflags(write=False)
    return dict(frames=np.stack([p[0] for p in pages])[:, None], polys=[p[1] for p in pages], where=[p[2] for p in pages],
                adj=[[1.0, 1.0]] * len(pages), words=words, table=table, logits=x, blank=blank, beam=beam, images=list(imgs))
