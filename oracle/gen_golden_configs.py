"""Generate tests/golden/reference_configs.json: for every config file of the REFERENCE's own ``configs/`` tree, what the model
builders read from it -- ``task``, ``model``, ``data.sparse`` and ``data.eval.input_shape`` as ``Config.fromfile`` returns them --
and, for the in-scope families, the name, shape and dtype of every entry of the reference model's ``state_dict()`` (the
reference's ``build_model``, dmb/modeling/__init__.py:10, imported as oracle/gen_golden.py does).  Fixtures are data: the
tests rebuild this package's ``build_model(cfg)`` from the recorded settings and load the recorded state dict ``strict=True``
(tests/test_host_logic.py), so they no longer need the reference tree.

    PYTHONDONTWRITEBYTECODE=1 python oracle/gen_golden_configs.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from oracle.gen_golden import OUT, REF, import_reference, load_cfg  # noqa: E402

IN_SCOPE = ("PSMNet", "AcfNet", "StereoNet", "GCNet")


def settings(cfg):
    """The parts of a config file the model builders read (densematchingbenchmark_amd/modeling: cfg.task, cfg.model,
    cfg.data.sparse) and the input shape the tests check; nothing of the data sets' locations."""
    data = cfg.get("data", {})
    return {"task": cfg.get("task", "stereo"), "model": cfg["model"],
            "data": {"sparse": data.get("sparse", False), "eval": {"input_shape": list(data["eval"]["input_shape"])}}}


def main():
    from densematchingbenchmark_amd.config import Config
    from densematchingbenchmark_amd.modeling import build_model
    import_reference()
    from dmb.modeling import build_model as ref_build_model
    out = {}
    for fam in sorted(os.listdir(os.path.join(REF, "configs"))):
        d = os.path.join(REF, "configs", fam)
        if not os.path.isdir(d):
            continue
        for f in sorted(os.listdir(d)):
            if not f.endswith(".py"):
                continue
            rel = "configs/%s/%s" % (fam, f)
            rec = {"family": fam, "in_scope": fam in IN_SCOPE,
                   "settings": json.loads(json.dumps(settings(Config.fromfile(os.path.join(REF, rel)))))}
            if fam in IN_SCOPE:
                sd = ref_build_model(load_cfg(rel)).state_dict()
                rec["state_dict"] = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()]
                # the recorded settings must build what the file itself builds (JSON turns tuples into lists)
                a = build_model(Config.fromfile(os.path.join(REF, rel))).state_dict()
                b = build_model(Config(rec["settings"])).state_dict()
                assert [(k, tuple(v.shape)) for k, v in a.items()] == [(k, tuple(v.shape)) for k, v in b.items()], rel
            out[rel] = rec
    path = os.path.join(OUT, "reference_configs.json")
    with open(path, "w") as fp:
        fp.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in out.items()) + "\n}\n")
    print("%s: %d configs, %.1f KB" % (path, len(out), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
