"""Drop-in conformance GENERATED from the reference's two caller scripts (CPU).

train_transformed_rays.py (TR) and eval_transformed_rays.py (EV) are parsed with `ast` by oracle/make_golden.py (`dropin`), which
stores in tests/golden/dropin_reference.json every name they import from `nerf` (TR:17-21, EV:30-39), every call they make to one
of those names -- positional arity and keyword names --, every `getattr(models, cfg.models.<net>.type)(...)` construction
(TR:100-124, EV:274-299), the signatures of the public functions, every model `type:` the shipped YAML configs name and the
state_dict schema of the in-scope families.  The product package must accept each of them (inspect.signature(...).bind).
Nothing here is typed in by hand: if a script passes a keyword the product does not take, this test names the call site.  Where
the reference tree is present, the stored record is checked against a fresh extraction."""
import inspect
import json
import os

import pytest
import torch

from oracle import make_golden as MG
from oracle import ref_import as RI

SCRIPTS = MG.DROPIN_SCRIPTS
IN_SCOPE_MODELS = MG.DROPIN_MODELS
RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dropin_reference.json")


def _record():
    with open(RECORD) as f:
        return json.load(f)


def _product():
    import nerf
    return nerf


@pytest.mark.parametrize("script", SCRIPTS)
def test_every_imported_name_exists(script):
    import importlib
    nerf = _product()
    names = _record()["scripts"][script]["imports"]
    assert names, "no nerf imports found: the parser is looking at the wrong file"
    for local, (module, attr) in names.items():
        mod = nerf if module == "nerf" else importlib.import_module(module)      # e.g. `from nerf.load_flame import ...` (TR:17)
        assert mod.__file__.startswith(os.path.dirname(nerf.__file__)), (module, mod.__file__)   # the PRODUCT package, not the reference
        assert hasattr(mod, attr), f"{script}: `from {module} import {attr}` has no counterpart in the product package"


@pytest.mark.parametrize("script", SCRIPTS)
def test_every_call_site_binds(script):
    nerf = _product()
    rec = _record()["scripts"][script]
    names, calls = rec["imports"], rec["calls"]
    seen = {c[0] for c in calls}
    assert {"run_one_iter_of_nerf", "get_ray_bundle", "get_embedding_function", "<model>"} <= seen, seen
    for callee, n_pos, kws, line in calls:
        if callee.startswith("<model>"):
            classes = [callee.split(":", 1)[1]] if ":" in callee else list(IN_SCOPE_MODELS)
            for cls in classes:
                if cls not in IN_SCOPE_MODELS:
                    continue                      # a hard-coded construction of an out-of-scope ablation class
                sig = inspect.signature(getattr(nerf.models, cls).__init__)
                try:
                    sig.bind(None, *([None] * n_pos), **{k: None for k in kws})
                except TypeError as e:
                    pytest.fail(f"{script}:{line}: models.{cls}(...) does not accept the script's arguments: {e}")
            continue
        module, attr = names[callee]
        obj = getattr(nerf, attr) if module == "nerf" else getattr(__import__(module, fromlist=[attr]), attr)
        try:
            inspect.signature(obj).bind(*([None] * n_pos), **{k: None for k in kws})
        except TypeError as e:
            pytest.fail(f"{script}:{line}: {attr}(...) does not accept the script's arguments: {e}")


def test_run_one_iter_signature_is_the_references():
    """Same parameter names, order and defaults as T:165-181 (taken from the reference's own function objects)."""
    nerf = _product()
    empty = inspect.Parameter.empty
    for fn, params in _record()["signatures"].items():
        pa = [(p[0], p[1] if len(p) > 1 else empty) for p in params]
        b = inspect.signature(getattr(nerf, fn))
        pb = [(p.name, p.default) for p in b.parameters.values()]
        assert [n for n, _ in pa] == [n for n, _ in pb][:len(pa)], (fn, pa, pb)
        for (n, da), (_, db) in zip(pa, pb):
            assert (da is empty) == (db is empty) and (da is empty or da == db), (fn, n, da, db)
        assert all(d is not empty for _, d in pb[len(pa):]), fn      # extensions must be optional


def test_model_types_of_the_shipped_configs():
    """Every `type:` under `models:` in the reference's config/*.yml: the two in-scope families must be constructible with the
    trainer's keyword set (and produce the reference's state_dict keys and shapes); the rest are listed as out of scope."""
    rec = _record()
    nerf = _product()
    types = rec["config_model_types"]
    assert sum(types.values()) > 50 and set(IN_SCOPE_MODELS) <= set(types), types
    covered = sum(n for t, n in types.items() if t in IN_SCOPE_MODELS)
    print(f"model types in shipped configs: {types}; fused HIP path covers {covered} of {sum(types.values())} entries")
    for t in IN_SCOPE_MODELS:
        sa = {k: torch.zeros(shape) for k, shape in rec["state_dicts"][t]}
        b = getattr(nerf.models, t)(**MG.DROPIN_MODEL_KW)
        sb = b.state_dict()
        assert list(sa) == list(sb) and all(sa[k].shape == sb[k].shape for k in sa), t
        b.load_state_dict(sa)                                       # a reference checkpoint's keys and shapes load unchanged
    assert covered >= 0.85 * sum(types.values())


@pytest.mark.skipif(not RI.reference_available(), reason="the reference tree is not present here")
def test_record_equals_live_reference():
    """tests/golden/dropin_reference.json is what oracle/make_golden.py extracts from the reference tree today."""
    assert MG.dropin_record(RI.import_reference()) == _record()
