"""What the Python wrappers of the pipeline stages (unitig_filter, scrubber, kmer_filter, unitigs, mapper) share: the
exception with its one message format, the view of a result's text, and the create / run / read the error / free the
result / destroy sequence around ``msgpu_<prefix>_*``."""
import contextlib
import ctypes as C

from . import _lib

__all__ = ["StageError", "text_view", "stage_context"]


class StageError(RuntimeError):
    """A rejected input or a device failure of a stage; ``line`` = 1-based line (0: none) of input ``file``."""

    def __init__(self, code, file=0, line=0, detail=""):
        msg = _lib.lib().msgpu_strerror(code).decode()
        where = self.where(file, line) if line else ""
        super().__init__("%s (%d)%s%s" % (msg, code, where, (": " + detail) if detail else ""))
        self.code = code
        self.file = file
        self.line = line

    @staticmethod
    def where(file, line):
        """how a stage names a place in its inputs"""
        return " (file %d line %d)" % (file, line)


def text_view(fn, res, which=None):
    """a view of one of a result's texts, or of its only one (valid until the result is freed)"""
    n = C.c_uint64()
    p = fn(res, C.byref(n)) if which is None else fn(res, which, C.byref(n))
    return memoryview((C.c_char * n.value).from_address(p)) if n.value else b""


class _Stage:
    def __init__(self, L, prefix, ctx, error_cls):
        self.L, self.prefix, self.ctx, self.error_cls = L, prefix, ctx, error_cls

    def _fn(self, name):
        return getattr(self.L, "msgpu_%s_%s" % (self.prefix, name), None)

    def check(self, rc):
        """raises the stage's exception, with what the context says about it, when a run returned a code"""
        if rc == _lib.OK:
            return
        where = {key: int(self._fn("error_" + key)(self.ctx)) for key in ("line", "file") if self._fn("error_" + key)}
        raise self.error_cls(rc, detail=self._fn("last_error")(self.ctx).decode(errors="replace"), **where)

    @contextlib.contextmanager
    def run(self, *args, fn="run"):
        """``msgpu_<prefix>_<fn>(ctx, *args, &result)``: the result, freed on the way out"""
        res = C.c_void_p()
        self.check(self._fn(fn)(self.ctx, *args, C.byref(res)))
        try:
            yield res
        finally:
            self._fn("result_free")(res)


@contextlib.contextmanager
def stage_context(prefix, device, error_cls):
    """``msgpu_<prefix>_create`` ... ``_destroy`` around the block; yields the stage, whose ``run`` raises ``error_cls``"""
    L = _lib.lib()
    stage = _Stage(L, prefix, C.c_void_p(), error_cls)
    rc = stage._fn("create")(device, C.byref(stage.ctx))
    if rc != _lib.OK:
        raise error_cls(rc, detail="device %d" % device)
    try:
        yield stage
    finally:
        stage._fn("destroy")(stage.ctx)
