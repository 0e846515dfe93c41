"""CPU: tests/stream_cases.py against include/cofhe_hip.h -- every entry of the header with a parameter called `stream` has a
stream case or stands in the short list of exclusions with its reason, and nothing else does.  An entry point added later
without a stream case fails here.  No kernel runs."""
import os
import re

import stream_cases as SC
from conftest import ROOT
from test_engine_signatures_cpu import header_prototypes

# what may be excluded at all: entries that make, end, probe or fence a stream, that move host memory, that time, or that need
# a communicator
MAY_BE_EXCLUDED = {"cofhe_hip_stream_create", "cofhe_hip_stream_destroy", "cofhe_hip_stream_query", "cofhe_hip_stream_sync", "cofhe_hip_upload",
                   "cofhe_hip_download", "cofhe_hip_timer_start", "cofhe_hip_timer_stop", "cofhe_hip_time_compose", "cofhe_hip_all_gather_rows"}


def stream_entries():
    """the names of the prototypes of the header that have a parameter named `stream`, parsed as header_prototypes() does"""
    text = open(os.path.join(ROOT, "include", "cofhe_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", " ", text, flags=re.M)
    names = set()
    for stmt in re.split(r"[;{}]", text):
        m = re.fullmatch(r"\s*(.*?)\s*\b(cofhe_hip_\w+)\s*\(([^()]*)\)\s*", stmt, flags=re.S)
        if not m:
            continue
        params = [re.sub(r"\[[^\]]*\]", "", p).split() for p in m.group(3).split(",")]
        if any(p and p[-1].lstrip("*") == "stream" for p in params):
            names.add(m.group(2))
    return names


def test_the_parser_sees_what_the_signature_test_sees():
    protos = header_prototypes()
    found = stream_entries()
    assert found <= set(protos)
    assert len(found) >= 60
    assert {"cofhe_hip_compose_records", "cofhe_hip_stream_create", "cofhe_hip_unpack_tensor_device", "cofhe_hip_timer_stop"} <= found
    assert not {"cofhe_hip_malloc", "cofhe_hip_free", "cofhe_hip_view_check", "cofhe_hip_add_ciphertext_tensors_bytes"} & found
    for name in found:                                       # a stream is a pointer wherever it stands
        assert "p" in protos[name].split(":")[1], name


def test_every_stream_entry_has_a_case_or_a_reason():
    found = stream_entries()
    assert sorted(found - set(SC.TABLE) - set(SC.EXCLUDED)) == [], "entries with a stream and no stream case"
    assert sorted(set(SC.TABLE) - found) == [], "cases of entries that take no stream"
    assert sorted(set(SC.EXCLUDED) - found) == [], "exclusions of entries that take no stream"
    assert sorted(set(SC.TABLE) & set(SC.EXCLUDED)) == []


def test_the_exclusions_are_the_allowed_ones_with_reasons():
    assert set(SC.EXCLUDED) <= MAY_BE_EXCLUDED
    for name, why in SC.EXCLUDED.items():
        assert isinstance(why, str) and len(why.split()) >= 3, name


def test_variants_name_table_entries():
    assert set(SC.VARIANTS) <= set(SC.TABLE)
    ids = SC.case_ids()
    assert len(ids) == len(set(ids)) == len(SC.TABLE) + sum(len(v) - 1 for v in SC.VARIANTS.values())
    for name, build in SC.TABLE.items():
        assert callable(build), name
