"""Stand-ins for the host tests of the detector's object columns: the resident set of
tests/test_iterative_batch_host.py with set_detect_objects, whose detect() then adds scripted columns that name their own
row, and a context that records what extract_objects hands to scene_detect_objects.  No GPU is touched."""
import numpy as np

from tests import test_iterative_batch_host as bh

DET = ("npix", "peak", "flux", "xmin", "xmax", "ymin", "ymax", "x2", "y2", "xy", "a", "b", "theta", "flag")
INT = ("npix", "xmin", "xmax", "ymin", "ymax", "flag")


def scripted_column(name, passes, n):
    """column `name` of the detect() call number `passes` with n rows: every value names its column, its pass and its row"""
    v = 1000.0 * (DET.index(name) + 1) + 100.0 * passes + np.arange(n)
    return v.astype(np.int32) if name in INT else v + 0.25


class ObjectsSet(bh.ScriptedSet):
    def __init__(self, owner, fields, cumulative):
        super().__init__(owner, fields, cumulative)
        self.objects_on = False

    def set_detect_objects(self, on=True, segmentation_map=False):
        self.owner.calls.append(("set_detect_objects", bool(on), bool(segmentation_map)))
        self.objects_on = bool(on)

    def detect(self, active=None, **kw):
        out = super().detect(active=active)
        if self.objects_on:
            n = len(out["x"])
            out.update({name: scripted_column(name, self.k, n) for name in DET})
        return out


class ObjectsEngine(bh.StubEngine):
    def open_field_set(self, fields, cumulative=False):
        self.calls.append(("open", bool(cumulative)))
        self.sets.append(ObjectsSet(self, np.asarray(fields), cumulative))
        return self.sets[-1]


def batch(script):
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch

    net = bh.Net(script)
    net._core.engine = ObjectsEngine(script)
    fields = np.random.default_rng(1).normal(size=(len(script), bh.F, bh.F, bh.NB))
    return IterativeDeblendFieldBatch(net, fields, bh.CS, bh.NB), net._core.engine


class RecordingContext:
    """scene_detect_objects of two fields with 2 and 1 objects: columns that name their row"""

    def scene_detect_objects(self, fields, **kw):
        from debvader_amd import engine as E

        self.shape, self.kw = np.shape(fields), kw
        n = 3
        out = dict(offsets=np.array([0, 2, 3], np.int64), globalrms=np.ones(2))
        for i, k in enumerate(("field", "parent", "npix") + E.OBJECT_KEYS[:9]):
            out[k] = (100 * i + np.arange(n)).astype(np.int32)
        for i, k in enumerate(("peak", "flux", "x", "y") + E.OBJECT_KEYS[9:]):
            out[k] = 0.5 + 10.0 * i + np.arange(n)
        out.update(E.detect_object_shapes(out["x2"], out["y2"], out["xy"]))
        if kw.get("segmentation_map"):
            out["segmap"] = np.arange(2 * fields.shape[1] * fields.shape[2], dtype=np.int32).reshape((2,) + fields.shape[1:3])
        return out
