"""The public surface of voxelhashing_amd.engine, held to a fixture written from the commit before the module became a
package: every public name, the signature and docstring of every function and of every class's public methods.

Needs neither a GPU nor the built library: importing the package loads nothing.

    python tests/test_engine_surface.py --write     # records the surface of the checked-out tree in the fixture
"""
import hashlib
import inspect
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_surface.json")
ALIASES = ("C", "np")  # import aliases, not part of the surface
ALWAYS = ("__init__", "close", "__del__")  # recorded for a class beside its public methods, where the class has them
NEW_PUBLIC = ()  # public names added since the fixture was written; the modules of the package are found by themselves


def _callable_record(fn):
    doc = inspect.getdoc(fn)
    return {"signature": str(inspect.signature(fn)), "doc": hashlib.sha256(doc.encode()).hexdigest() if doc else None}


def _class_record(cls):
    methods = {}
    for name in dir(cls):
        if name.startswith("_") and name not in ALWAYS:
            continue
        raw = inspect.getattr_static(cls, name)
        if isinstance(raw, (staticmethod, classmethod)):
            raw = raw.__func__
        if not inspect.isfunction(raw):
            continue  # (object's slot wrappers, class attributes)
        methods[name] = dict(_callable_record(raw), static=isinstance(inspect.getattr_static(cls, name), staticmethod))
    doc = inspect.getdoc(cls)
    return {"kind": "class", "doc": hashlib.sha256(doc.encode()).hexdigest() if doc else None, "methods": methods}


def _from_engine(obj, engine):
    mod = getattr(obj, "__module__", None) or ""
    return mod == engine.__name__ or mod.startswith(engine.__name__ + ".")


def surface(engine):
    """-> {name: record} of every attribute that does not start with an underscore, the aliases and the package's own
    modules excepted"""
    out = {}
    for name, obj in sorted(vars(engine).items()):
        if name.startswith("_") or name in ALIASES:
            continue
        if isinstance(obj, types.ModuleType):
            if obj.__name__.startswith(engine.__name__ + "."):
                continue  # a module of the package itself
            out[name] = {"kind": "module"}
        elif not _from_engine(obj, engine):
            out[name] = {"kind": "reexport"}  # a name of lib: DeviceBuffer, load, ...
        elif inspect.isclass(obj):
            out[name] = _class_record(obj)
        elif inspect.isfunction(obj):
            out[name] = dict(_callable_record(obj), kind="function")
        else:
            out[name] = {"kind": type(obj).__name__}
    return out


def _engine():
    from voxelhashing_amd import engine
    return engine


def test_importing_the_engine_does_not_load_the_library():
    import subprocess
    code = "import sys; sys.path.insert(0, %r); from voxelhashing_amd import engine, lib; assert lib._LIB is None" % ROOT
    subprocess.run([sys.executable, "-c", code], check=True)


def test_public_names_are_those_of_the_fixture():
    with open(FIXTURE) as f:
        want = json.load(f)
    have = surface(_engine())
    assert sorted(set(want) - set(have)) == [], "public names that went missing"
    assert sorted(set(have) - set(want)) == sorted(NEW_PUBLIC), "public names the fixture does not know"


def test_signatures_and_docstrings_are_those_of_the_fixture():
    with open(FIXTURE) as f:
        want = json.load(f)
    have = surface(_engine())
    changed = []
    for name, rec in want.items():
        got = have.get(name)
        if got is None or got["kind"] != rec["kind"]:
            changed.append(name)
        elif rec["kind"] == "function" and got != rec:
            changed.append(name)
        elif rec["kind"] == "class":
            if got["doc"] != rec["doc"]:
                changed.append(name)
            changed += [f"{name}.{m}" for m in sorted(set(rec["methods"]) | set(got["methods"])) if rec["methods"].get(m) != got["methods"].get(m)]
    assert changed == []


def test_lib_names_and_modules_stay_reachable():
    E = _engine()
    from voxelhashing_amd import canonical, lib, vhtypes
    for name in ("DeviceBuffer", "load", "VhError", "check", "download", "f16"):
        assert getattr(E, name) is getattr(lib, name)
    assert E.T is vhtypes and E.canonical is canonical


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit(__doc__)
    with open(FIXTURE, "w") as f:
        json.dump(surface(_engine()), f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {FIXTURE}")
