"""forced.chunk_posterior without a GPU, on hand-made finished chunks: a chunk with nothing to refine, a page off the
array path, the mapping of the per-syllable array through `indices`, and PagePosterior's two constructors."""
import numpy as np

from forced_post_ref import same_bits


class _Chunk(object):
    """what chunk_posterior reads of a finished alignToOCR.PageChunk"""

    def __init__(self, transcripts, lines_per_page, post):
        self.transcripts, self.post = transcripts, post
        self._first = np.concatenate([[0], np.cumsum(lines_per_page)]).astype(np.int64)

    def first_line(self):
        return self._first


def test_a_chunk_with_nothing_to_refine_has_no_values():
    from text_alignment_amd import forced
    out = forced.chunk_posterior(_Chunk(["abc de", "", "xy"], [2, 0, 1], None), [[0, 1], [], [0]])
    assert [type(o) for o in out] == [forced.PagePosterior] * 3
    assert [len(o.char_posterior) for o in out] == [6, 0, 2]
    assert all(o.char_posterior.dtype == np.float64 and np.isnan(o.char_posterior).all() for o in out)
    assert [o.syllable_posterior for o in out] == [[None, None], [], [None]]
    for name in ("posterior", "rival_posterior", "posterior_rival", "loglik_bits"):
        assert [getattr(o, name) for o in out] == [[None, None], [], [None]], name


def test_indices_pick_the_boxes_values_and_an_object_path_page_has_none():
    from text_alignment_amd import forced
    nan = np.nan
    # page 0: two lines, the second not aligned; four syllables of which the boxes show 3, 0 and 1 (1 has no value).
    # page 1: off the array path -- the device reduced no syllable for it.  page 2: no line at all.
    post = {"posterior": [np.array([0.5, 0.25]), None, np.array([1.0])],
            "rival_posterior": [np.array([0.25, 0.5]), None, np.array([0.0])],
            "posterior_rival": [np.array([0, 4], np.int32), None, np.array([2], np.int32)],
            "loglik_bits": [-3.5, None, -0.25],
            "char": [np.array([0.5, 0.25, nan, nan]), np.array([nan, 1.0, nan]), np.zeros(0)],
            "syllable": [np.array([0.25, nan, 5e-324, 0.0]), np.zeros(0), np.zeros(0)]}
    out = forced.chunk_posterior(_Chunk(["abcd", "xyz", ""], [2, 1, 0], post), [[3, 0, 1], [0, 0], []])
    assert out[0].syllable_posterior == [0.0, 0.25, None] and [type(v) for v in out[0].syllable_posterior[:2]] == [float] * 2
    assert out[1].syllable_posterior == [None, None] and out[2].syllable_posterior == []
    assert same_bits(out[0].char_posterior, post["char"][0]) and same_bits(out[1].char_posterior, post["char"][1])
    assert len(out[0].posterior) == 2 and out[0].posterior[1] is None and same_bits(out[0].posterior[0], [0.5, 0.25])
    assert out[0].loglik_bits == [-3.5, None] and out[1].loglik_bits == [-0.25] and out[2].loglik_bits == []
    assert out[1].posterior_rival[0].tolist() == [2] and out[0].rival_posterior[1] is None
    # a subnormal value is a value
    one = forced.chunk_posterior(_Chunk(["abcd"], [2], dict(post, syllable=[post["syllable"][0]], char=[post["char"][0]])), [[2]])
    assert one[0].syllable_posterior == [5e-324]


def test_page_posterior_is_still_made_from_a_refine_result():
    from text_alignment_amd import forced

    class _H(object):
        line_first = [0, 1, 3]

    class _Res(object):
        harvest = _H()
        char_posterior, syllable_posterior = ["c0", "c1"], ["s0", "s1"]
        posterior, rival_posterior, posterior_rival, loglik_bits = [1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12]
    p = forced.PagePosterior(_Res(), 1)
    assert (p.char_posterior, p.syllable_posterior, p.posterior, p.rival_posterior, p.posterior_rival, p.loglik_bits) == (
        "c1", "s1", [2, 3], [5, 6], [8, 9], [11, 12])
    q = forced.PagePosterior.of("c", "s", [1], [2], [3], [4])
    assert type(q) is forced.PagePosterior
    assert (q.char_posterior, q.syllable_posterior, q.posterior, q.rival_posterior, q.posterior_rival, q.loglik_bits) == (
        "c", "s", [1], [2], [3], [4])
