"""The Python half of a network handle of libga3c_hip.so, for what the four networks' classes do word for word alike
behind the entries <PREFIX>_* (NetworkVP.Network, NetworkVP_vector.Network, NetworkVP_discrate.Network,
NetworkDDPG.Network): NativeHandle is what all four share, ParamHandle adds the arenas and the variables by name of the
three actor-critic networks (DDPG's param_info has another signature).  The table behind both is the one of
csrc/ga3c_vartable.hpp."""
import ctypes as C
import glob
import os
import re

import numpy as np

from Config import Config
import _native as nat


class NativeHandle:
    """A subclass states PREFIX and sets _lib, _h, model_name and, where its rows are vectors, S."""
    PREFIX = None                 # the entries are <PREFIX>_create, <PREFIX>_train, ...

    def _fn(self, entry):
        return getattr(self._lib, "%s_%s" % (self.PREFIX, entry))

    def _call(self, entry, *args):
        """<PREFIX>_<entry>(handle, *args), checked."""
        return nat.check(self._fn(entry)(self._h, *args), "%s_%s" % (self.PREFIX, entry))

    def close(self):
        if getattr(self, "_h", None):
            self._fn("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _rows(self, x):
        x = nat.as_f32(x).reshape(-1, self.S)
        return x, int(x.shape[0])

    def get_global_step(self):
        s = C.c_int64()
        nat.check(self._fn("get_step")(self._h, C.byref(s)))
        return s.value

    def get_variables_names(self):
        n = self._fn("num_params")(self._h)
        return [self._fn("param_name")(self._h, i).decode() + ":0" for i in range(n)]

    # ---- zero-copy intake from the shared-memory transport (rows of 4 S bytes) -------------------
    def register_transport(self, transport):
        self._call("register_host", C.c_void_p(transport.base), transport.nbytes)

    def unregister_transport(self):
        self._call("unregister_host")

    def gather_entry(self):
        """(address of <PREFIX>_predict_gather, handle, u8 = 0) for the native predictor loop (ga3c_pq_serve)."""
        return C.cast(self._fn("predict_gather"), C.c_void_p).value, self._h, 0

    def gather_entries_pipelined(self):
        """(addresses of <PREFIX>_predict_gather_begin / _end, handle, u8 = 0) for ga3c_pq_serve_pipelined."""
        return (C.cast(self._fn("predict_gather_begin"), C.c_void_p).value,
                C.cast(self._fn("predict_gather_end"), C.c_void_p).value, self._h, 0)

    def fetch(self, name, count):
        out = np.empty(int(count), np.float32)
        self._call("fetch", name.encode(), nat.ptr(out), out.size)
        return out

    def _checkpoint_filename(self, episode):
        return 'checkpoints/%s_%08d' % (self.model_name, episode)

    def save(self, episode):
        """An .npz keyed by the TF variable names, their optimizer slots and the step, written by the library itself
        (<PREFIX>_save): a TF checkpoint cannot be written without TF."""
        os.makedirs("checkpoints", exist_ok=True)
        self._call("save", (self._checkpoint_filename(episode) + ".npz").encode())

    def load_file(self, filename):
        self._call("load", filename.encode())

    def load(self):
        if Config.LOAD_EPISODE > 0:
            filename = self._checkpoint_filename(Config.LOAD_EPISODE) + ".npz"
        else:
            found = sorted(glob.glob('checkpoints/%s_????????.npz' % self.model_name))
            if not found:
                raise FileNotFoundError("no checkpoint for %s" % self.model_name)
            filename = found[-1]
        self.load_file(filename)
        return int(re.split(r'/|_|\.', filename[:-4])[2])


class ParamHandle(NativeHandle):
    """A subclass also sets param_count, the arena's floats."""

    # ---- arenas: 0 weights, 1 / 2 RMSProp `ms` / `mom`, 3 last gradient; with Config.DUAL_RMSPROP (where the network takes
    # it) these are cost_p's optimizer and 4 / 5 / 6 the value optimizer's `ms` / `mom` and the last cost_v gradient ------
    def get_arena(self, which):
        out = np.empty(self.param_count, dtype=np.float32)
        self._call("get_arena", which, nat.ptr(out), out.size)
        return out

    def set_arena(self, which, flat):
        flat = nat.as_f32(flat).ravel()
        self._call("set_arena", which, nat.ptr(flat), flat.size)

    def _param_info(self, name):
        off, count, ndim = C.c_int64(), C.c_int64(), C.c_int32()
        shape = (C.c_int64 * 4)()
        self._call("param_info", name.encode(), C.byref(off), C.byref(count), C.byref(ndim), shape)
        return off.value, count.value, tuple(shape[d] for d in range(ndim.value))

    def get_variable_value(self, name, which=0):
        _, count, shape = self._param_info(name)
        out = np.empty(count, dtype=np.float32)
        self._call("get_param", name.encode(), which, nat.ptr(out), count)
        return out.reshape(shape)

    def set_variable_value(self, name, value, which=0):
        flat = nat.as_f32(value).ravel()
        self._call("set_param", name.encode(), which, nat.ptr(flat), flat.size)
