"""Integer bookkeeping of a factor graph (vipe/slam/components/factor_graph.py:66-75) on the host, so that the scheduling
logic around the update iteration - duplicate filtering, suppression, age eviction, plan building - reads no device
memory back.  The device tensors the reference keeps are made from the host arrays on request, one array at a time."""

import numpy as np
import torch

from .._lib import upload

NAMES = ("ii", "jj", "age", "ii_inac", "jj_inac")  # active edges and their age; edges moved to the inactive store


def as_host(x, dtype=np.int64):
    """tensor, list or array -> flat numpy array of `dtype` (a device tensor is read back)"""
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return x.astype(dtype).reshape(-1)


class EdgeIndex:
    """Owns the five int64 arrays `host[name]` and the set of all edges; its methods are the only code that edits them."""

    def __init__(self, device):
        self._device = device
        self.version = 0  # counts edits of the edge lists (an `age` tick is none)
        self.host = {n: np.zeros(0, dtype=np.int64) for n in NAMES}
        self._dev = dict.fromkeys(NAMES)  # device tensor per array; None: to be uploaded
        self._set = set()  # {(i, j)} of all active + inactive edges; None: rebuilt on next use

    def _put(self, **arrays):
        for n, a in arrays.items():
            a.flags.writeable = False  # handed out as they are: nobody edits them in place
            self.host[n], self._dev[n] = a, None
        self.version += arrays.keys() != {"age"}

    def device(self, name):
        """the device tensor of one array: uploaded on demand, the same tensor until THAT array changes"""
        if self._dev[name] is None:
            self._dev[name] = upload(self.host[name], self._device)
        return self._dev[name]

    def assign(self, name, tensor):
        """`graph.<name> = tensor` from outside: replaces that array only (one read-back); when `ii` changes its length,
        `age` restarts at zero"""
        a = as_host(tensor)
        if name == "ii" and a.shape[0] != self.host["ii"].shape[0]:
            self._put(age=np.zeros_like(a))
        self._put(**{name: a})
        self._dev[name] = tensor
        if name != "age":
            self._set = None

    def edge_set(self):
        """{(i, j)} of all edges, kept in step by the mutators (the inactive list grows with the video: rebuilding the
        set per call is O(length of the video) of Python per keyframe); a batch that repeated an edge leaves the count
        out of step: rebuilt then"""
        h = self.host
        if self._set is None or len(self._set) != h["ii"].shape[0] + h["ii_inac"].shape[0]:
            self._set = set(zip(h["ii"].tolist(), h["jj"].tolist())) | set(zip(h["ii_inac"].tolist(), h["jj_inac"].tolist()))
        return self._set

    def absent(self, ii, jj):
        """the edges of (ii, jj) that are neither active nor inactive (factor_graph.py:96-108: a .item() per edge there)"""
        have = self.edge_set()
        keep = np.array([(i, j) not in have for i, j in zip(ii.tolist(), jj.tolist())], dtype=bool)
        return ii[keep], jj[keep]

    def append(self, ii, jj):
        """new active edges, age 0"""
        h = self.host
        self.edge_set().update(zip(ii.tolist(), jj.tolist()))
        self._put(ii=np.concatenate([h["ii"], ii]), jj=np.concatenate([h["jj"], jj]),
                  age=np.concatenate([h["age"], np.zeros_like(ii)]))

    def remove(self, mask, store):
        """drop the active edges of the bool `mask`; with `store` they go to the end of the inactive list"""
        h = self.host
        if store:
            self._put(ii_inac=np.concatenate([h["ii_inac"], h["ii"][mask]]), jj_inac=np.concatenate([h["jj_inac"], h["jj"][mask]]))
        elif self._set is not None:
            self._set.difference_update(zip(h["ii"][mask].tolist(), h["jj"][mask].tolist()))
        self._put(ii=h["ii"][~mask], jj=h["jj"][~mask], age=h["age"][~mask])

    def drop_keyframe(self, ix):
        """keyframe `ix` leaves the buffer, the frames behind it move up one place.  -> bool masks (active, inactive) of
        the edges that touched it: the inactive ones are dropped here, the active ones are left to the caller's `remove`
        (their per-edge tensors go with them)"""
        h = self.host
        active, inactive = (h["ii"] == ix) | (h["jj"] == ix), (h["ii_inac"] == ix) | (h["jj_inac"] == ix)
        self._put(ii=h["ii"] - (h["ii"] >= ix), jj=h["jj"] - (h["jj"] >= ix),
                  ii_inac=(h["ii_inac"] - (h["ii_inac"] >= ix))[~inactive], jj_inac=(h["jj_inac"] - (h["jj_inac"] >= ix))[~inactive])
        self._set = None
        return active, inactive

    def tick(self):
        self._put(age=self.host["age"] + 1)  # factor_graph.py:306
