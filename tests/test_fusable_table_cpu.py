"""The pure-host coverage queries (mg_modconv_dgrad_fusable, mg_conv2d_wgrad_bias_fusable,
mg_gemm_wgrad_bias_fusable) give, over the grid of tools/fusable_table.py and under each of its tuning settings, the
answers recorded in tests/fusable_table.json by the commit before the dispatch plans (csrc/mg_plan.h): moving the
dispatch rules behind one module changed no answer.  No device is touched."""
import importlib.util
import json
import os

import pytest

from conftest import PKG, REPO


def test_fusable_answers_match_recorded_table():
    path = os.path.join(PKG, "moegan_mi", "libmoegan_hip.so")
    if not os.path.exists(path):
        pytest.skip("libmoegan_hip.so not built (run __graft_entry__.build())")
    spec = importlib.util.spec_from_file_location("fusable_table", os.path.join(REPO, "tools", "fusable_table.py"))
    ft = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ft)
    with open(os.path.join(REPO, "tests", "fusable_table.json")) as f:
        want = json.load(f)
    got = ft.table(ft.load(path))
    assert list(got) == list(want)
    for setting in want:
        assert want[setting]["n"] == got[setting]["n"] > 10000, setting
        assert 0 < want[setting]["ones"] or setting == "11=1", setting  # the grid reaches covered calls
        assert got[setting] == want[setting], f"tuning {setting}: the answers differ from the recorded ones"
