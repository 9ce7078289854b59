"""Stand-ins for the host tests of the detector's cleaning pass: the resident set of
tests/stub_detect_objects_engine.py with set_detect_clean, whose detect() then adds a scripted nmerged, and a context that
records what the detection module hands to scene_detect / scene_detect_objects / scene_detect_clean.  No GPU is touched."""
import numpy as np

from tests import stub_detect_objects_engine as so
from tests import test_iterative_batch_host as bh


def scripted_nmerged(passes, n):
    """nmerged of the detect() call number `passes` with n rows: every value names its pass and its row"""
    return (7000 + 100 * passes + np.arange(n)).astype(np.int32)


class CleanSet(so.ObjectsSet):
    def __init__(self, owner, fields, cumulative):
        super().__init__(owner, fields, cumulative)
        self.clean_on = False

    def set_detect_clean(self, on=True, clean_param=1.0):
        self.owner.calls.append(("set_detect_clean", bool(on), float(clean_param)))
        self.clean_on = bool(on)

    def detect(self, active=None, **kw):
        out = super().detect(active=active, **kw)
        if self.clean_on:
            n = len(out["x"])
            out.update(nmerged=scripted_nmerged(self.k, n), mthresh=np.full(n, 0.25), n_raw=np.zeros(self.fields.shape[0], np.int64))
        return out


class CleanEngine(bh.StubEngine):
    def open_field_set(self, fields, cumulative=False):
        self.calls.append(("open", bool(cumulative)))
        self.sets.append(CleanSet(self, np.asarray(fields), cumulative))
        return self.sets[-1]


def batch(script):
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch

    net = bh.Net(script)
    net._core.engine = CleanEngine(script)
    fields = np.random.default_rng(1).normal(size=(len(script), bh.F, bh.F, bh.NB))
    return IterativeDeblendFieldBatch(net, fields, bh.CS, bh.NB), net._core.engine


class RecordingContext(so.RecordingContext):
    """two fields with 2 and 1 objects; `called` names the entry point, kw what it got"""

    def scene_detect(self, fields, **kw):
        self.called = "scene_detect"
        out = so.RecordingContext.scene_detect_objects(self, fields, **kw)
        return out

    def scene_detect_multiband(self, fields, **kw):
        self.called = "scene_detect_multiband"
        return so.RecordingContext.scene_detect_objects(self, fields, **kw)

    def scene_detect_objects(self, fields, **kw):
        self.called = "scene_detect_objects"
        return super().scene_detect_objects(fields, **kw)

    def scene_detect_clean(self, fields, **kw):
        out = so.RecordingContext.scene_detect_objects(self, fields, **kw)
        self.called = "scene_detect_clean"
        out.update(nmerged=np.array([3, 1, 2], np.int32), mthresh=np.array([0.25, 0.5, 0.75]), n_raw=np.array([4, 2], np.int64))
        return out
