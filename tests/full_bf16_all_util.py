"""Helpers of tests/test_gpu_full_bf16_all.py.

private_copy(name) loads tests/<name>.py as a module object of its OWN, under another module name: the comparisons of an
existing GPU test file (tests/test_gpu_full_language.py, whose functions find their engines through the module global
new_engine) can then run on bf16 engines by setting that global in the copy.  The module pytest collects is another
object and is never touched, so nothing depends on test order, on fixture teardown or on how pytest names modules, and
the dictionaries a copy fills (test_gpu_full_bf16.observed) are not the ones the collected file reports."""
import importlib.util
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def private_copy(name):
    spec = importlib.util.spec_from_file_location("full_bf16_all_copy_of_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def bf16_engine_factory(plain, default_positions):
    """new_engine(pkg, fix, language, positions, **opts) of tests/test_gpu_full_language.py with the three options of the
    bf16 storage mode set behind the caller's."""

    def new_engine(pkg, fix, language=-1, positions=default_positions, **opts):
        return plain(pkg, fix, language, positions, **dict(opts, bf16=1, full_bf16=1, full_bf16_all=1))

    return new_engine
