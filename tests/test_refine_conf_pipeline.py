"""forced.chunk_confidence without a GPU, on hand-made finished chunks (the counterpart of test_refine_post_pipeline.py):
a chunk with nothing to refine, a page off the array path, the mapping of the per-syllable array through `indices`
(picked, repeated, out of order) and NO_CONFIDENCE -> None."""
import numpy as np


class _Chunk(object):
    """what chunk_confidence reads of a finished alignToOCR.PageChunk"""

    def __init__(self, transcripts, lines_per_page, conf):
        self.transcripts, self.conf = transcripts, conf
        self._first = np.concatenate([[0], np.cumsum(lines_per_page)]).astype(np.int64)

    def first_line(self):
        return self._first


def test_a_chunk_with_nothing_to_refine_has_no_values():
    from text_alignment_amd import forced
    out = forced.chunk_confidence(_Chunk(["abc de", "", "xy"], [2, 0, 1], None), [[0, 1], [], [0]])
    assert [type(o) for o in out] == [forced.PageConfidence] * 3
    assert [len(o.char_confidence) for o in out] == [6, 0, 2]
    assert all(o.char_confidence.dtype == np.int64 and (o.char_confidence == forced.NO_CONFIDENCE).all() for o in out)
    assert [o.syllable_confidence for o in out] == [[None, None], [], [None]]
    for name in ("confidence", "rival"):
        assert [getattr(o, name) for o in out] == [[None, None], [], [None]], name


def test_indices_pick_the_boxes_values_and_an_object_path_page_has_none():
    from text_alignment_amd import forced
    none = forced.NO_CONFIDENCE
    # page 0: two lines, the second not aligned; four syllables of which the boxes show 3, 0, 1 and 3 again (1 has no
    # value).  page 1: off the array path -- the device reduced no syllable for it.  page 2: no line at all.
    conf = {"confidence": [np.array([70000, -3], np.int64), None, np.array([0], np.int64)],
            "rival": [np.array([0, 4], np.int32), None, np.array([2], np.int32)],
            "char": [np.array([70000, -3, none, none], np.int64), np.array([none, 0, none], np.int64), np.zeros(0, np.int64)],
            "syllable": [np.array([-3, none, 70000, 0], np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)]}
    out = forced.chunk_confidence(_Chunk(["abcd", "xyz", ""], [2, 1, 0], conf), [[3, 0, 1, 3], [0, 0], []])
    assert out[0].syllable_confidence == [0, -3, None, 0]
    assert [type(v) for v in out[0].syllable_confidence] == [int, int, type(None), int]
    assert out[1].syllable_confidence == [None, None] and out[2].syllable_confidence == []
    for p in range(3):
        assert out[p].char_confidence.dtype == np.int64 and out[p].char_confidence.tolist() == conf["char"][p].tolist()
    assert len(out[0].confidence) == 2 and out[0].confidence[1] is None and out[0].confidence[0].tolist() == [70000, -3]
    assert len(out[0].rival) == 2 and out[0].rival[1] is None and out[0].rival[0].tolist() == [0, 4]
    assert [c.tolist() for c in out[1].confidence] == [[0]] and [r.tolist() for r in out[1].rival] == [[2]]
    assert out[2].confidence == [] and out[2].rival == []
    # the most negative value but one is a value
    one = forced.chunk_confidence(_Chunk(["abcd"], [2], dict(conf, syllable=[np.array([none + 1, none], np.int64)],
                                                             char=[conf["char"][0]])), [[0, 1, 0]])
    assert one[0].syllable_confidence == [none + 1, None, none + 1]
