"""CPU: TrainPipeline's schedule policy (lipasr/schedule.py) pinned to the rules the constructor applied inline before the split.
The expected values were worked out by hand from that code, not taken from plan_schedule."""
import ast
import os

import pytest

from lipasr import knobs
from lipasr.schedule import plan_schedule

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "asr-using-robust-nn_amd", "lipasr")
REST = lambda cus, tiles=128: ("rest", cus, tiles, cus)   # classifier, train_cus, GEMM tile threshold, CU budget
OWN, POOL = ("own_queue", None, None, None), ("pool", None, None, None)
F16 = dict(batch=1024, compute_dtype="float16x2")
F32 = dict(batch=1024, compute_dtype="float32")

# (arguments, environment, extraction CUs, classifier, graph, flags wanted, wide wanted, Adam signal)
CASES = {
    "b1024-f16x2": (F16, {}, 128, REST(128), False, True, True, True),
    "b1024-f32": (F32, {}, 96, REST(160), False, True, True, True),
    "b512-f32": (dict(batch=512), {}, 64, REST(192), False, True, True, True),
    "b2048-f16x2": (dict(batch=2048, compute_dtype="float16x2"), {}, 128, REST(128), False, True, True, True),
    "per-layer": (dict(F32, constraint="per_layer"), {}, 96, REST(160), False, True, True, False),
    "pgd": (dict(F32, pgd=True), {}, 128, OWN, True, True, True, False),
    "custom-extractor": (dict(F32, custom_extractor=True), {}, 224, OWN, False, True, False, True),
    "no-partition": (dict(F32, mfcc_cus=None), {}, None, POOL, False, True, False, True),
    "no-partition-pgd": (dict(F32, mfcc_cus=None, pgd=True), {}, None, OWN, True, True, False, False),
    "share-above-chip": (dict(F32, mfcc_cus=300), {}, None, POOL, False, True, False, True),
    "share-40": (dict(F32, mfcc_cus=40), {}, 32, REST(224), False, True, True, True),
    "share-16-floor": (dict(F32, mfcc_cus=16), {}, 32, REST(224), False, True, True, True),
    "world-2": (dict(F16, world=2), {}, 128, REST(128), False, False, True, False),
    "env-mfcc-cus": (F32, {"LIPASR_MFCC_CUS": "160"}, 160, REST(96), False, True, True, True),
    "env-train-all": (F32, {"LIPASR_TRAIN_CUS": "all"}, 128, OWN, False, True, True, True),
    "env-no-own-queue-pgd": (dict(F32, pgd=True), {"LIPASR_TRAIN_OWN_QUEUE": "0"}, 128, POOL, True, True, True, False),
    "env-events": (F16, {"LIPASR_GPU_FLAGS": "0"}, 128, REST(128), False, False, True, False),
    "env-gemm-tiles": (F32, {"LIPASR_GEMM_TILES": "96"}, 96, REST(160, tiles=96), False, True, True, True),
    "304-cus": (dict(F32, n_cu=304), {}, 96, REST(208), False, True, True, True),
    # beyond the table: the one place where the two former copies of "rest or all" disagreed -- PGD sent to the rest of the chip
    # by the variable kept the shared schedule's half for the extraction, by the argument it gets the share measured for "rest"
    "env-train-rest-pgd": (dict(F32, pgd=True), {"LIPASR_TRAIN_CUS": "rest"}, 128, REST(128), True, True, True, False),
    "arg-train-rest-pgd": (dict(F32, pgd=True, train_cus="rest"), {}, 96, REST(160), True, True, True, False),
    "explicit-graph-sync-bn": (dict(F32, world=2, sync_bn=True, use_graph=False), {}, 96, REST(160), False, False, True, False),
    "auto-graph-sync-bn": (dict(F32, world=2, sync_bn=True), {}, 96, REST(160), True, False, True, False),
    "no-adam-entry-point": (dict(F32, has_adam_signal=False), {}, 96, REST(160), False, True, True, False),
    "env-flags-on-world-2": (dict(F16, world=2), {"LIPASR_GPU_FLAGS": "1"}, 128, REST(128), False, True, True, False),
    "env-narrow": (F32, {"LIPASR_WIDE_WHEN_IDLE": "0"}, 96, REST(160), False, True, False, True),
    "env-adam-signal-off": (F32, {"LIPASR_ADAM_SIGNAL": "0"}, 96, REST(160), False, True, True, False),
}


@pytest.fixture
def clean_env(monkeypatch):
    for row in knobs.TABLE:
        monkeypatch.delenv(row.name, raising=False)
    return monkeypatch


@pytest.mark.parametrize("case", CASES)
def test_plan_schedule_follows_the_constructor_rules(clean_env, case):
    args, env, mfcc_cus, (classifier, train_cus, tiles, budget), graph, flags, wide, adam = CASES[case]
    for k, v in env.items():
        clean_env.setenv(k, v)
    s = plan_schedule(**dict(dict(n_cu=256), **args))
    n_cu = args.get("n_cu", 256)
    assert s.mfcc_cus == mfcc_cus and s.mfcc_groups == (None if mfcc_cus is None else mfcc_cus // 8)
    assert s.classifier == classifier and s.train_cus == (train_cus if classifier == "rest" else n_cu)
    assert (s.gemm_tiles, s.cu_budget) == (tiles, budget)
    assert (s.use_graph, s.flags, s.wide, s.adam_signal) == (graph, flags, wide, adam)
    groups = s.classifier_groups
    assert groups == {"rest": (s.mfcc_groups, n_cu // 8), "own_queue": (0, n_cu // 8), "pool": None}[classifier]


def test_without_cu_masking_the_plan_is_the_unpartitioned_one(clean_env):
    """What the constructor does when the extraction's masked stream cannot be made: it plans again with mfcc_cus=None.  No
    partition, no wide stream; PGD still asks for a queue of its own; the flags stay a wish that only a masked classifier stream
    grants (TrainPipeline.__init__: flags and the Adam signal need that stream, the wide stream needs the extraction's)."""
    plain = plan_schedule(n_cu=256, mfcc_cus=None, **F16)
    assert (plain.mfcc_groups, plain.classifier, plain.classifier_groups, plain.wide) == (None, "pool", None, False)
    assert plain.flags and plain.adam_signal and plain.train_cus == 256
    pgd = plan_schedule(n_cu=256, mfcc_cus=None, pgd=True, **F16)
    assert (pgd.mfcc_groups, pgd.classifier, pgd.wide, pgd.use_graph) == (None, "own_queue", False, True)


def test_unparsable_integer_raises(clean_env):
    clean_env.setenv("LIPASR_MFCC_CUS", "many")
    with pytest.raises(ValueError):
        plan_schedule(n_cu=256, **F32)


def test_schedule_and_knobs_import_neither_torch_nor_the_native_library():
    for name in ("schedule.py", "knobs.py"):
        tree = ast.parse(open(os.path.join(PKG, name)).read())
        mods = set()
        for node in ast.walk(tree):
            if isinstance(node, ast.Import):
                mods |= {a.name.split(".")[0] for a in node.names}
            elif isinstance(node, ast.ImportFrom):
                mods |= {node.module.split(".")[0]} if node.module else {a.name for a in node.names}
        assert mods <= {"dataclasses", "typing", "os", "knobs"}, (name, mods)
