"""json_extract_kernel (n1k_jsondev.hip) document by document.

No ABI call returns the device-extracted columns, so every document carries a unique "id" and the plan groups by it:
each group is then one document, and after_items_raw() hands back its values — tag plus 64 payload bits, string codes
resolved through dict_get (json_util.Channel).  Every comparison is three-way and bit-exact:

  1. the Python reference computed from the document's text (json_util.reference_values; checked against the host
     extractor without a GPU in test_json_reference_cpu.py);
  2. the host route: the same plan and the same process_json calls with json_device=0 — the control for the channel: if
     IT disagrees with the reference, the grouping channel or the reference is at fault, not the kernel;
  3. the device route: json_device=1, json_device_min_docs=1.

json_device_docs (documents the kernel typed itself) is asserted exactly, against json_util.stays_on_device() — the
hand-over rules restated from the kernel's header comment — or against the generator's labels."""
import numpy as np
import pytest

import json_util as ju
import query_amd
from query_amd import _ffi, plan

pytestmark = pytest.mark.gpu


def _halves(docs):
    """two process_json calls where there is more than one document: strings first interned by the first batch and met
    again in the second go through the remap twice"""
    return [docs] if len(docs) < 2 else [docs[:len(docs) // 2], docs[len(docs) // 2:]]


def three_way(channel, batches, device_docs, **options):
    """Runs both routes over the batches; asserts the three-way equality and the device's document count.  `device_docs`:
    a number, or None = what stays_on_device() predicts.  Returns the device route's statistics."""
    docs = [d for b in batches for d in b]
    want = channel.expected(docs)
    host, hst = channel.run(batches, 0, **options)
    diff = ju.first_difference(host, want)
    assert diff is None, "the HOST route disagrees with the reference (the channel or the reference is at fault): " + diff
    assert hst["json_device_docs"] == 0
    dev, dst = channel.run(batches, 1, **options)
    diff = ju.first_difference(dev, want)
    assert diff is None, "the device route disagrees with the reference and the host route: " + diff
    if device_docs is None:
        paths = [("id",)] + channel.key_paths + channel.agg_paths
        device_docs = ju.predicted_device_docs(batches, paths) if ju.paths_on_device(paths) else 0
    assert dst["json_device_docs"] == device_docs, (dst["json_device_docs"], device_docs, len(docs))
    return dst


# ------------------------------------------------------------------------------------------------ number literals

NUMBERS = ju.Channel([("a",)], [("b",)])  # a comes back as a group key, b through MIN


@pytest.mark.parametrize("seed", range(8))
def test_number_literals_typed_on_the_device(seed):
    """Run 1: only literals of the device's kind (json_util.number_on_device) — every document is typed by the kernel's own
    arithmetic: the 18-digit integers, Clinger's exact case, the fold to INT."""
    docs = ju.number_docs(seed, 4096, device_only=True)
    three_way(NUMBERS, _halves(docs), len(docs))


@pytest.mark.parametrize("seed", range(8))
def test_number_literals_mixed(seed):
    """Run 2: every literal of the generator; the kernel hands over exactly the documents stays_on_device() predicts."""
    docs = ju.number_docs(seed, 4096)
    st = three_way(NUMBERS, _halves(docs), None, json_device_left_pct=100)
    assert 0.1 * len(docs) < st["json_device_docs"] < 0.6 * len(docs)  # (both numbers of a document must be the device's kind)


# ------------------------------------------------------------------------------------------------------ structure

STRUCT = ju.Channel(ju.STRUCT_KEYS, ju.STRUCT_AGGS)


@pytest.mark.parametrize("seed", range(6))
def test_random_structure(seed):
    """Documents generated as text: whitespace, duplicates at every level, wanted names in skipped values, prefix /
    extension names, escaped names before and after the paths are found, the string sizes and repeats of the issue's
    list; the device keeps exactly the documents the generator labels device-kind."""
    docs, labels = ju.structure_docs(seed, 2048)
    three_way(STRUCT, _halves(docs), int(np.sum(labels)), json_device_left_pct=100)


def _plain_docs(n, first=0):
    """small device-kind documents with few distinct strings"""
    return [('{"id": "d%d", "s": "%s", "price": %d.5, "x": {"y": %d, "z": "%s"}, "w": {"y": true}}'
             % (i, "abc"[i % 3] * (i % 5), i % 7, i, "st%d" % (i % 11))).encode() for i in range(first, first + n)]


def test_prefix_paths():
    """`x` and `x.y` in one plan: with x a scalar the kernel takes x and leaves x.y MISSING; with x an object the document
    is the host's (canonical text)."""
    ch = ju.Channel([("x",), ("x", "y")])
    scalar = [b'{"id": "d%d", "x": %s}' % (i, v) for i, v in enumerate([b"5", b'"str"', b"null", b"1.5", b"true"] * 20)]
    three_way(ch, _halves(scalar), len(scalar))
    obj = [b'{"id": "o%d", "x": {"y": %d, "z": [1.0, "a"]}}' % (i, i) for i in range(70)] + [b'{"id": "e", "x": {}}', b'{"id": "m"}']
    three_way(ch, [obj], 1, json_device_left_pct=100)  # (only the document without x stays)
    mixed = [d for pair in zip(scalar[:70], obj[:70]) for d in pair]
    three_way(ch, _halves(mixed), 70, json_device_left_pct=100)


def test_sibling_paths():
    """x.y, x.z and w.y: the kernel descends, returns and descends again at the same level; x and w in either order, twice,
    with the wanted names at other levels too."""
    ch = ju.Channel([], [("x", "y"), ("x", "z"), ("w", "y")])
    shapes = ['{"id": "d%d", "x": {"y": %d, "z": "z%d"}, "w": {"y": 1.25}}', '{"id": "d%d", "w": {"y": %d, "z": "no"}, "x": {"z": "z%d", "y": -1}}',
              '{"id": "d%d", "x": {"z": %d}, "y": "top", "w": {"x": {"y": "deep"}, "y": "w%d"}, "x": {"y": "second x"}}',
              '{"id": "d%d", "y": 1, "z": 2, "w": {}, "x": {"z": %d, "y": %d}}',
              '{"id": "d%d", "x": {"x": {"y": 0, "z": 0}, "w": {"y": 0}, "y": %d}, "w": {"w": {"y": 0}, "y": %d, "y": 3}}']
    docs = [(shapes[i % len(shapes)] % (i, i, i % 13)).encode() for i in range(300)]
    three_way(ch, _halves(docs), len(docs))


def test_path_depth():
    """A 4-step path runs on the device; a 5-step path and an array-element path are refused as a whole."""
    docs = [('{"id": "d%d", "a": {"b": {"c": {"d": %d, "e": {"f": "five%d"}}, "l": [10, "e%d", {"d": 1}]}, "d": "no"}}' % (i, i, i % 9, i % 7)).encode()
            for i in range(150)] + [b'{"id": "s", "a": {"b": {"c": 5}}}', b'{"id": "t", "a": {"b": {"c": {"d": "leaf"}}}}']
    three_way(ju.Channel([("a", "b", "c", "d")]), _halves(docs), len(docs))
    three_way(ju.Channel([("a", "b", "c", "d")], [("a", "b", "c", "e", "f")]), _halves(docs), 0)
    three_way(ju.Channel([("a", "b", "c", "d")], [("a", "b", "l", 1)]), _halves(docs), 0)
    three_way(ju.Channel([("a", "b", "l", -1, "d")]), _halves(docs), 0)


def _columns_plan(ncond):
    cond = None
    for i in range(ncond):  # (true for every document, whatever c<i> holds)
        term = "((%s is missing) or (%s is not missing))" % (ju.D("c%d" % i), ju.D("c%d" % i))
        cond = term if cond is None else "(%s and %s)" % (cond, term)
    return ju.Channel([("k1",), ("k2",), ("k3",)], [("a%d" % i, "v") for i in range(8)], condition=cond)


def test_sixteen_leaf_columns():
    """kMaxCols: 4 keys, 8 aggregate operands and 4 condition columns in one plan, all extracted on the device."""
    ch = _columns_plan(4)
    docs = []
    for i in range(200):
        m = ['"id": "d%d"' % i, '"k1": %d' % (i % 5), '"k2": "s%d"' % (i % 3), '"k3": %s' % ["true", "null", "1.5"][i % 3]]
        m += ['"a%d": {"v": %s}' % (j, ['"t%d"' % (i % 4), str(i * j), "%d.25" % j, "false"][(i + j) % 4]) for j in range(8) if (i + j) % 9]
        m += ['"c%d": %d' % (j, i) for j in range(4) if (i >> j) & 1]
        docs.append(("{" + ", ".join(m[i % 3:] + m[:i % 3]) + "}").encode())
    op = query_amd.GpuFilterGroup(ch.plan)
    assert len(op.column_paths) == 16
    op.done()
    # (the condition columns are read by the kernel too — stays_on_device() sees them all)
    assert all(ju.stays_on_device(d, [("id",)] + ch.key_paths + ch.agg_paths + [("c%d" % j,) for j in range(4)]) for d in docs)
    three_way(ch, _halves(docs), len(docs))


def test_a_seventeenth_leaf_column_is_refused_by_n1k_create():
    with pytest.raises(query_amd.N1kError) as ei:
        query_amd.GpuFilterGroup(_columns_plan(5).plan)
    assert ei.value.status == _ffi.UNSUPPORTED and "more than 16 leaf paths" in ei.value.message


def _staging_batch(extra):
    """For a in 0..15: a filler that ends at an offset with offset % 16 == a, then a document of kJsonWaveBytes - 16 - a
    (+ extra) bytes starting there, then a small one."""
    docs, at = [], 0
    for a in range(16):
        size = 48 + (a - at - 48) % 16
        docs.append(ju.padded_doc(len(docs), size, tail=', "s": "f%d"' % a))
        at += size
        assert at % 16 == a
        big = ju.WAVE_BYTES - 16 - a + extra
        docs.append(ju.padded_doc(len(docs), big, tail=', "s": "edge", "x": {"y": %d.5}' % a))
        at += big
        docs.append(ju.padded_doc(len(docs), 60, tail=', "x": {"y": "after"}'))
        at += 60
    return docs


STAGING = ju.Channel([("s",)], [("x", "y")])


def test_staging_documents_that_fill_the_lds_share_exactly():
    """A document of kJsonWaveBytes - 16 - a bytes at an offset with offset % 16 == a fills the wave's share to the last
    byte (staged from the 16-byte boundary below its start) and is still the device's — for every a."""
    docs = _staging_batch(0)
    three_way(STAGING, [docs], len(docs))


def test_staging_documents_one_byte_over_the_lds_share():
    """One byte more and the document is the host's, alone in its sub-batch; its neighbours stay."""
    docs = _staging_batch(1)
    assert ju.predicted_device_docs([docs], [("id",), ("s",), ("x", "y")]) == len(docs) - 16
    three_way(STAGING, [docs], len(docs) - 16, json_device_left_pct=100)


def test_staging_a_large_document_between_small_ones():
    """A 20 000-byte document between two 20-byte ones inside one wave: the sub-batch before it ends, it goes to the host
    (cnt == 0), the next sub-batch starts behind it."""
    small = lambda i: b'{"id":"d%d","s":"ab"}' % i
    assert len(small(0)) == 20
    docs = [small(0), ju.padded_doc(1, 20000), small(2)]
    three_way(STAGING, [docs], 2, json_device_left_pct=100)
    docs = [small(i) for i in range(10, 40)] + [ju.padded_doc(1, 20000), small(2), ju.padded_doc(3, 20000), ju.padded_doc(4, 16000), small(5)]
    three_way(STAGING, [docs], len(docs) - 2, json_device_left_pct=100)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_document_counts(n):
    """Less than a wave, a wave to the document, one more, and more than a workgroup's four waves."""
    docs = _plain_docs(n)
    three_way(ju.Channel([("s",), ("price",)], [("x", "y"), ("x", "z"), ("w", "y")]), _halves(docs), n)


def test_nonzero_base():
    """offsets[0] == 7 and seven bytes of junk before the first document: the same result (the kernel stages from
    16-byte boundaries of the bytes it was given, not of the caller's buffer)."""
    docs = _staging_batch(0)[:9] + _plain_docs(130, first=1000)
    three_way(ju.Channel([("s",)], [("x", "y")]), _halves(docs), len(docs), nonzero_base=7)


@pytest.mark.parametrize("nhost,kept", [(136, True), (137, False)])
def test_whole_batch_hand_over(nhost, kept):
    """push_json_device: more than ndocs * json_device_left_pct / 100 + 16 documents left to the host and the host path
    takes the whole batch — 1000 documents at 12 %: 136 are patched in, 137 are not."""
    docs = _plain_docs(1000)
    step = 1000 // nhost
    for j in range(nhost):  # an escape in a wanted string: the host's
        docs[j * step] = b'{"id": "d%d", "s": "tab\\there", "x": {"y": %d}}' % (j * step, j)
    ch = ju.Channel([("s",)], [("x", "y")])
    assert ju.predicted_device_docs([docs], [("id",), ("s",), ("x", "y")]) == 1000 - nhost
    three_way(ch, [docs], 1000 - nhost if kept else 0, json_device_left_pct=12)


# ------------------------------------------------------------------------------------------- malformed documents

MALFORMED = {"truncated": '{"id": "bad", "s": "v", "k": [1, 2', "trailing comma": '{"id": "bad", "s": "v", "k": 1,}',
             "bad literal": '{"id": "bad", "s": %s}' % "tru", "bad escape": '{"id": "bad", "s": "a\\qb"}',
             "unquoted name": '{"id": "bad", s: "v"}', "trailing bytes": '{"id": "bad", "s": "v"} x',
             "1.": '{"id": "bad", "s": 1.}', "-": '{"id": "bad", "s": -}', "1e": '{"id": "bad", "s": 1e}'}


def _expect_invalid(docs, index, device):
    op = query_amd.GpuFilterGroup(ju.Channel([("s",)], [("x", "y")]).plan, json_device=device, json_device_min_docs=1)
    try:
        with pytest.raises(query_amd.N1kError) as ei:
            op.process_json(docs)
    finally:
        op.done()
    assert ei.value.status == _ffi.INVALID and ("document %d " % index) in ei.value.message + " ", (device, ei.value.message)


@pytest.mark.parametrize("kind", sorted(MALFORMED))
def test_malformed_document_in_the_middle_of_a_wave(kind):
    """Each kind of damage at a lane in the middle of a wave of good documents, once in a wanted value and once in a value
    that is only skipped: both routes answer N1K_INVALID and name that document."""
    at = 64 + 37
    for text in (MALFORMED[kind], MALFORMED[kind].replace('"s"', '"unwanted"').replace(" s:", " unwanted:")):
        docs = _plain_docs(200)
        docs[at] = text.encode()
        for device in (1, 0):
            _expect_invalid(docs, at, device)


def test_empty_document_is_named_as_malformed():
    docs = _plain_docs(100)
    docs[41] = b""
    for device in (1, 0):
        _expect_invalid(docs, 41, device)


def test_two_malformed_documents_the_lower_is_named():
    docs = _plain_docs(300)
    docs[280] = MALFORMED["trailing comma"].encode()
    docs[70] = MALFORMED["1e"].encode()
    docs[199] = MALFORMED["bad escape"].encode()
    for device in (1, 0):
        _expect_invalid(docs, 70, device)


def test_leading_zeros_are_taken_by_both_routes_alike():
    """`01` and `-007` are accepted by both extractors (Go's scanner would refuse the document: DESIGN.md §8 item 7).  No
    reference here: pinned is that the routes agree, and that the kernel keeps such documents."""
    docs = _plain_docs(100)
    docs[10] = b'{"id": "z1", "s": 01, "x": {"y": -007}}'
    docs[75] = b'{"id": "z2", "s": -00.50, "k": 00, "x": {"y": 0012e1}}'
    ch = ju.Channel([("s",)], [("x", "y")])
    host, hst = ch.run(_halves(docs), 0)
    dev, dst = ch.run(_halves(docs), 1)
    assert ju.first_difference(dev, host) is None and len(dev) == 100
    assert dev[b"z1"] == ((ju.T_INT, 1), (ju.T_INT, (-7) & ju.U64)) and dev[b"z2"][1] == (ju.T_INT, 120)
    assert hst["json_device_docs"] == 0 and dst["json_device_docs"] == 100
