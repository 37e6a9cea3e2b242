"""A recording stand-in for the Minimizer's device: a DeviceMesh and a mesh mirror that write down what they are handed,
in one ordered list, and refuse nothing.  The host tests of the module wiring share it (install_stub), and the
configuration log of tests/golden/minimizer_config_log.json is recorded with it."""

import numpy as np

from membrane_solver_amd import _lib as L
from membrane_solver_amd.geometry.mesh import _body_facet_mask


class Refused(Exception):
    """raised by a stub built with refuse=True for anything but obtaining the device"""


class RecordingDevice:
    """A DeviceMesh that records (name, args, kwargs) of every call and keeps the few values the Minimizer reads back:
    ``modules`` (set_params), ``fixed_plane``, ``perimeter_key`` / ``perimeter_loops`` and ``area_constraint``."""

    def __init__(self, calls, refuse=False):
        self.calls, self.modules, self.nv, self._refuse = calls, 0, 0, refuse
        self.fixed_plane = self.perimeter_key = self.area_constraint = None
        self.perimeter_loops = 0

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        if self._refuse and name != "set_deterministic":
            raise Refused("device call " + name)

        def rec(*a, **k):
            self.calls.append((name, a, k))
            if name == "set_params":
                self.modules = k["modules"]
            elif name == "set_fixed_plane":
                self.fixed_plane = (tuple(float(v) for v in a[0]), tuple(float(v) for v in a[1])) if a else None
            elif name == "set_perimeter":
                self.perimeter_key = tuple(np.asarray(v).tobytes() for v in a) if a else None
                self.perimeter_loops = len(a[3]) if a else 0
            elif name == "set_area_constraint":
                self.area_constraint = (int(a[0]), float(a[1])) if a[0] != L.MS_AREA_NONE else None
        return rec


class RecordingMirror:
    """What the Minimizer uses of geometry.mesh.MeshMirror; its calls go into the device's list under their own names."""

    def __init__(self, refuse=False):
        self.calls = []
        self.dm = RecordingDevice(self.calls, refuse)
        self.mesh, self.body, self._topo_key, self._leaflet_keys, self._refuse = None, None, 1, {}, refuse

    def sync(self, positions=None):
        if not self._refuse:
            self.calls.append(("sync", (), {}))
        if self.mesh is not None:
            tri, _ = self.mesh.triangle_row_cache()
            self.dm.nv = len(self.mesh.vertex_ids)
            self.body = _body_facet_mask(self.mesh, 0 if tri is None else len(tri))[1]
        return self.dm

    def _topology_key(self):
        return self._topo_key

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        if self._refuse:
            raise Refused("mirror call " + name)
        return lambda *a, **k: self.calls.append((name, a, k))


def install_stub(monkeypatch, refuse=False):
    """Make ``minimizer.mirror_for`` hand out one recording mirror -> (device, mirror); ``device.calls`` is the log.
    ``refuse``: every call but sync / set_deterministic raises Refused (for "refused before anything is uploaded")."""
    from membrane_solver_amd.runtime import minimizer as mzmod

    mir = RecordingMirror(refuse)

    def mirror_for(mesh, **_kw):
        mir.mesh = mesh
        return mir

    monkeypatch.setattr(mzmod, "mirror_for", mirror_for)
    return mir.dm, mir
