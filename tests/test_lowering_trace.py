"""tools/lowering_trace.py stays usable: the call trace of a lowering is reproducible, and a value it cannot render exactly
is an error rather than 'some object'.  (No golden digests: the tool compares two trees, see its docstring.)"""
import importlib.util
import os

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location(
    "lowering_trace", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "lowering_trace.py"))
LT = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(LT)
LT.use_root()


def test_trace_is_reproducible():
    digests = set()
    for name in ("concat_aligned", "blconv_bn"):
        for mode in ("f32", "bf16x3"):
            a, b = LT.trace_corpus(name, mode), LT.trace_corpus(name, mode)
            assert not isinstance(a, str) and len(a) > 5, (name, mode, a)
            assert any(r["calls"] for r in a)
            assert LT.digest(a) == LT.digest(b), (name, mode)
            digests.add(LT.digest(a))
    assert len(digests) == 4        # and it tells graphs and modes apart
    # a data-parallel step (sharded, embedded collectives) and the input pipeline: events and copies are traced too
    todo = LT.cases()
    for name in ("dp128/rs_ag/embedded/rank1", "pipeline128/resident"):
        a, b = todo[name](), todo[name]()
        assert any(r["pipe"] for r in a) and any(r["calls"] for r in a), name
        assert LT.digest(a) == LT.digest(b), name
        digests.add(LT.digest(a))
    assert len(digests) == 6


def test_unknown_value_type_is_an_error():
    assert LT.render((np.float32(1.5), [np.int64(3), None], {"a": (1, 'x')})) == [1.5, [3, None], {"a": [1, 'x']}]
    with pytest.raises(TypeError, match="unknown type object"):
        LT.render([1, object()])
    with pytest.raises(TypeError, match="unknown type function"):
        LT.render({"k": lambda: 0})
