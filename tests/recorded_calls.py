"""Test helper: the calls a piece of Python makes into libpam_hip.so, by entry name, in order."""
import contextlib


@contextlib.contextmanager
def recorded_calls():
    """Every call into libpam_hip.so, by name, in order."""
    from pam import _lib
    lib, calls, saved = _lib.load(), [], {}
    for name in _lib.EXPORTS:
        fn = getattr(lib, name)
        saved[name] = fn
        setattr(lib, name, (lambda f, nm: lambda *a: (calls.append(nm), f(*a))[1])(fn, name))
    try:
        yield calls
    finally:
        for name, fn in saved.items():
            setattr(lib, name, fn)
