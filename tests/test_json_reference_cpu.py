"""The generators and the text-level reference of tests/json_util.py against n1k_extract_json (host C++, no GPU), document
by document — before tests/test_gpu_json_device.py uses them to judge the device extractor — and stays_on_device() against
the labels the generators give by construction."""
import numpy as np
import pytest

import golden_util as gu
import json_util as ju
import query_amd
from query_amd import _ffi


def _extracted(channel, docs):
    """n1k_extract_json's values per document, in the order of channel.expected()"""
    op = query_amd.GpuFilterGroup(channel.plan)
    try:
        paths = [tuple(gu.path_steps(p)) for p in op.column_paths]
        cols = op.extract_json(docs)
        cache = {}

        def val(c, r):
            t, v = int(cols[c]["tags"][r]), int(cols[c]["payload"][r])
            if t >= ju.T_STRING:
                if v not in cache:
                    cache[v] = op.dict_get(v)
                return t, cache[v]
            return (t, v) if t in (ju.T_INT, ju.T_FLOAT) else (t, 0)

        want = [("id",)] + channel.key_paths + channel.agg_paths
        at = [paths.index(p) for p in want]
        return [[val(c, r) for c in at] for r in range(len(docs))], want
    finally:
        op.done()


def _assert_reference_is_the_extractor(channel, docs):
    got, want = _extracted(channel, docs)
    for r, doc in enumerate(docs):
        ref = ju.reference_values(doc, want)
        assert got[r] == ref, (r, doc[:300], got[r], ref)


NUMBERS = ju.Channel([("a",)], [("b",)])


@pytest.mark.parametrize("seed", range(8))
def test_number_literals_reference_is_the_host_extractor(seed):
    docs = ju.number_docs(seed, 4096)
    _assert_reference_is_the_extractor(NUMBERS, docs)
    dev = ju.number_docs(seed, 4096, device_only=True)
    _assert_reference_is_the_extractor(NUMBERS, dev)
    # the generator's device-only run is device-kind by the document rule too, and a mixed run is really mixed
    assert all(ju.stays_on_device(d, ju.NUMBER_PATHS) for d in dev[::16])
    share = np.mean([ju.number_on_device(x) for x in ju.number_literals(seed, 8192)])
    assert 0.3 < share < 0.7, share


def test_pinned_literals_are_typed_as_value_newvalue_types_them():
    I, F = ju.T_INT, ju.T_FLOAT
    bits = lambda f: int(np.float64(f).view(np.uint64))
    for lit, want in [(str(2 ** 53 + 1), (I, 2 ** 53 + 1)), (str(2 ** 63 - 1), (I, 2 ** 63 - 1)), (str(2 ** 63), (F, bits(2.0 ** 63))),
                      (str(-2 ** 63), (I, 2 ** 63)), (str(10 ** 18), (I, 10 ** 18)), ("1e18", (I, 10 ** 18)), ("1.0e18", (I, 10 ** 18)),
                      ("-0", (I, 0)), ("-0.0", (I, 0)), ("0e5", (I, 0)), ("1e22", (F, bits(1e22))), ("1e23", (F, bits(1e23))),
                      ("0.1", (F, bits(0.1))), ("0.30000000000000004", (F, bits(0.30000000000000004))), ("4.9e-324", (F, 1)),
                      ("1.5", (F, bits(1.5))), ("12.0", (I, 12)), ("-2.5e1", (I, (-25) & ju.U64))]:
        assert ju.type_number(lit) == want, lit


def test_number_rule_at_its_edges():
    on = ju.number_on_device
    assert on("123456789012345678") and not on("1234567890123456789")          # 18 / 19 digits, integer
    assert on("000000000000000000001") and on("-0") and on("0.000") and on("0e22") and not on("0e23")
    assert on("123456789012345.0e0") is False and on("12345678901234.0")       # trailing zeros are digits
    assert on("123456789012345e22") and not on("123456789012345e23")
    assert on("123456789012345e-22") and not on("123456789012345e-23")
    assert on("1.23456789012345e36") and not on("1.23456789012345e37")         # e10 = exponent - fraction digits
    assert on("1234567890123456") and not on("1234567890123456e0") and not on("1.234567890123456")
    assert on("0.0000000000000000000001") and not on("0.00000000000000000000001") and on("0.00000000000000000000001e1")
    assert not on("1.") and not on("-") and not on("1e") and not on("+1")


@pytest.mark.parametrize("seed", range(6))
def test_structure_documents_reference_is_the_host_extractor(seed):
    docs, labels = ju.structure_docs(seed, 2048)
    _assert_reference_is_the_extractor(ju.Channel(ju.STRUCT_KEYS, ju.STRUCT_AGGS), docs)
    offs = ju.batch_offsets(docs)
    for d, o, lab in zip(docs, offs, labels):
        assert ju.stays_on_device(d, ju.STRUCT_PATHS, o) == lab, (d, lab)
    assert 0.05 < 1 - np.mean(labels) < 0.5  # both kinds, mostly the device's
    # MIN operands are scalars by construction (no device path orders arrays / objects)
    na = len(ju.STRUCT_AGGS)
    assert all(t < ju.T_ARRAY for d in docs[::8] for t, _ in ju.reference_values(d, ju.STRUCT_AGGS)[:na])


def test_hand_over_rules_one_by_one():
    P = [("id",), ("s",), ("x", "y"), ("x", "z")]
    stay = lambda doc, paths=P, off=0: ju.stays_on_device(doc, paths, off)
    assert stay('{"id": "d0", "s": "v", "x": {"y": 1, "z": 2}}')
    assert stay(' {\n"id":"d0" ,\t"x" : { } , "s":null}\r\n') and stay("{}") and stay('{"x": 5, "s": true}')
    assert not stay("") and not stay("[1]") and not stay("7") and not stay('"s"')
    assert not stay('{"s": "a\\nb"}') and stay('{"k": "a\\nb", "s": "b"}') and stay('{"s": "b", "s": "a\\nb"}')
    assert not stay('{"s": [1]}') and not stay('{"s": {}}') and stay('{"s": 1, "s": [1]}') and stay('{"x": [1, {"y": [2]}]}')
    assert not stay('{"x": {"y": {"q": 1}}}') and not stay('{"x": {"y": 0.30000000000000004}}') and stay('{"k": 0.30000000000000004}')
    # escaped names: only where a path is still looked up
    assert not stay('{"\\u0073": 1}') and not stay('{"id": "d", "n\\n": 1, "s": 2, "x": {}}')
    assert stay('{"id": "d", "s": 2, "x": {}, "n\\n": 1}') and stay('{"k": {"n\\n": 1}, "s": 1}')
    assert not stay('{"x": {"y": 1, "\\u007a": 2, "z": 3}}') and stay('{"x": {"y": 1, "z": 3, "\\u007a": 2}}')
    # nesting of skipped values: 64 open non-empty brackets pass, 65 do not (empty ones do not count)
    assert stay('{"k": ' + "[" * 64 + "[]" + "]" * 64 + "}") and not stay('{"k": ' + "[" * 65 + "1" + "]" * 65 + "}")
    assert stay('{"x": {"k": ' + "[" * 64 + "1" + "]" * 64 + "}}")  # (counted per skipped value)
    # malformed
    for bad in ('{"s": 1', '{"s": 1,}', '{"s": tru}', '{"s": "\\q"}', '{s: 1}', '{"s": 1} x', '{"s": 1.}', '{"s": -}', '{"s": 1e}', '{"k": [1,]}'):
        assert not stay(bad), bad
    assert stay('{"s": 01, "k": -007}')  # (both scanners take leading zeros: DESIGN.md §8 item 7)
    # the wave's LDS share: len + offset % 16 <= kJsonWaveBytes - 16
    for a in range(16):
        size = ju.WAVE_BYTES - 16 - a
        assert stay(ju.padded_doc(0, size), P, 32 + a) and not stay(ju.padded_doc(0, size + 1), P, 32 + a)
    # the plan's side
    assert not stay("{}", [("a", "b", "c", "d", "e")]) and stay("{}", [("a", "b", "c", "d")]) and not stay("{}", [("a", 0)])
    assert not stay("{}", [("p%d" % i,) for i in range(17)]) and stay("{}", [("p%d" % i,) for i in range(16)])


def test_directed_documents_reference_is_the_host_extractor():
    docs = [b'{"id": "d0", "x": 5, "w": {"y": 1}}', b'{"id": "d1", "x": {"y": 1.5, "z": "s", "y": 2}, "w": {"y": true}, "x": {"y": 9}}',
            b'{"id": "d2", "x": {"z": 1e3}, "w": {"z": 1}}', b'{"id": "d3", "x": {"y": {"k": [1, 1.0, 1.50]}}}',
            b'{"id": "d4", "\\u0078": {"y": "esc"}, "x": {"y": "plain"}}', ju.padded_doc(5, 20000), b'{"id": "d6"}']
    _assert_reference_is_the_extractor(ju.Channel([("x",), ("x", "y")], [("x", "z"), ("w", "y")]), docs)


def test_directed_cases_of_the_gpu_tests_without_a_gpu(monkeypatch):
    """The directed GPU tests (tests/test_gpu_json_device.py) with their three-way check replaced by what can be known
    here: for every batch they push, the reference equals n1k_extract_json per document, and the document count they
    assert of the device is what stays_on_device() and push_json_device's whole-batch rule predict."""
    import test_gpu_json_device as T
    seen = []

    def on_the_cpu(channel, batches, device_docs, **options):
        docs = [d for b in batches for d in b]
        _assert_reference_is_the_extractor(channel, docs)
        paths = [("id",)] + channel.key_paths + channel.agg_paths
        total = 0
        if ju.paths_on_device(paths):
            for b in batches:
                stay = ju.predicted_device_docs([b], paths)
                if len(b) - stay <= len(b) * options.get("json_device_left_pct", 12) // 100 + 16:
                    total += stay
        assert device_docs is None or device_docs == total, (device_docs, total)
        seen.append((len(docs), total))
        return {"json_device_docs": total}

    monkeypatch.setattr(T, "three_way", on_the_cpu)
    T.test_prefix_paths()
    T.test_sibling_paths()
    T.test_path_depth()
    T.test_sixteen_leaf_columns()
    T.test_staging_documents_that_fill_the_lds_share_exactly()
    T.test_staging_documents_one_byte_over_the_lds_share()
    T.test_staging_a_large_document_between_small_ones()
    for n in (1, 63, 64, 65, 257):
        T.test_document_counts(n)
    T.test_nonzero_base()
    T.test_whole_batch_hand_over(136, True)
    T.test_whole_batch_hand_over(137, False)
    assert len(seen) == 21 and (1000, 864) in seen and (1000, 0) in seen
    # the malformed documents are malformed for the host extractor and for the rules
    op = query_amd.GpuFilterGroup(ju.Channel([("s",)], [("x", "y")]).plan)
    for text in T.MALFORMED.values():
        for t in (text, text.replace('"s"', '"unwanted"').replace(" s:", " unwanted:")):
            with pytest.raises(query_amd.N1kError) as ei:
                op.extract_json([b"{}", t.encode()])
            assert ei.value.status == _ffi.INVALID and "document 1 " in ei.value.message
            assert not ju.stays_on_device(t, [("id",), ("s",), ("x", "y")])
    op.done()
