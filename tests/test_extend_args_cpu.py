"""The Python side of the session calls without a GPU: the wrappers gpt.GPT offers, their defaults, and the bindings'
arity against the declarations of include/zgpt2.h."""
import inspect
import re

from zig_gpt2_amd import _lib
from zig_gpt2_amd import gpt as zgpt

NEW = ["zg_gpt_cached_len", "zg_gpt_extend", "zg_gpt_generate_from_enqueue", "zg_gpt_generate_fetch_range", "zg_debug_attn_prefill_at"]


def test_wrappers_and_defaults():
    p = inspect.signature(zgpt.GPT.generate_from).parameters
    assert list(p)[:4] == ["self", "past_len", "prompts", "n_steps"]
    assert p["temp"].default is None and p["seed"].default == 0 and p["top_k"].default == 0 and p["top_p"].default == 1.0
    assert list(inspect.signature(zgpt.GPT.extend).parameters)[:3] == ["self", "past_len", "tokens"]
    assert list(inspect.signature(zgpt.GPT.generate_fetch_range).parameters) == ["self", "first", "n"]
    assert list(inspect.signature(zgpt.GPT.cached_len).parameters) == ["self"]


def test_bindings_have_the_header_arity():
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/zgpt2.h"
        assert len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(",")), name
