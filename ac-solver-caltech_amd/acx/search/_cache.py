"""The solution cache of the searches scored by a caller's model (csrc/acx_cache.hip, C-ABI
acx_cache_* in include/acx.h): the dict of value_search/value_guided_search.py:100-250 --
backfill_solution_cache, _expand_cache_with_rotations, _check_cache_with_rotations -- as a hash set
of packed state keys that lives on the device across calls.

Only the states are on the device.  The paths stay here, verbatim: a backfilled path is kept once,
with its ordinal, and a cache entry says (path ordinal, step, relator, k), from which its value --
reversed(undo_moves) + path[step:] -- is made when someone asks for it.  An entry's rotation moves
are read off the entry's own key, so nothing is replayed on the host and nothing per entry crosses
on the way in."""

from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from . import _batch_bfs

# value_guided_search.py:119-122: (relator, generator g) -> the move r_i -> g r_i g^-1
CONJ_MOVE = {(0, 1): 7, (0, -1): 11, (0, 2): 9, (0, -2): 5, (1, 1): 8, (1, -1): 4, (1, 2): 10, (1, -2): 6}
_LETTER = np.array([1, -1, 2, -2], np.int8)  # a key's 2-bit codes (csrc/acx_key.h)
MAX_STEPS = 1 << 23  # a path's steps fit the entry's meta word (csrc/acx_cache.h)
DEFAULT_CAPACITY = 1024


def cache_bytes(L: int, capacity: int) -> int:
    """Device bytes of a cache of `capacity` rows at max_relator_length L (acx_cache_bytes):
    (8 kw + 8) C + 64 ceil(C / 4) + 16, kw = ceil((4L + 16) / 64).  No library call."""
    if not 1 <= L <= _lib.MAX_L or not 1 <= capacity <= 1 << 33:
        raise ValueError("L must be in [1, 128] and capacity in [1, 2^33]")
    return (8 * _lib.key_words(L) + 8) * capacity + 64 * ((capacity + 3) // 4) + 16


def unpack_keys(keys: np.ndarray, L: int) -> np.ndarray:
    """(M, kw) uint64 packed keys -> (M, 2L) int8 presentations (host; csrc/acx_key.h's format)"""
    keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1, _lib.key_words(L))
    bits = np.unpackbits(keys.view(np.uint8), axis=1, bitorder="little")
    codes = bits[:, 0:4 * L:2] | (bits[:, 1:4 * L:2] << 1)
    lens = np.packbits(bits[:, 4 * L:4 * L + 16].reshape(-1, 2, 8), axis=2, bitorder="little").reshape(-1, 2)
    out = _LETTER[codes]
    idx = np.arange(L)[None, :]
    out[:, :L][idx >= lens[:, :1]] = 0
    out[:, L:][idx >= lens[:, 1:]] = 0
    return out


def _rows_2d(states, L, what):
    """(N, 2L) int32 rows inside the packed domain, or ValueError"""
    if isinstance(states, torch.Tensor):
        states = states.detach().cpu().numpy()
    try:
        p = np.asarray(states)
    except ValueError as e:
        raise ValueError(f"{what} must be rows of equal length") from e
    if p.ndim == 1 and p.dtype != object and p.size == 2 * L:
        p = p.reshape(1, -1)
    if p.dtype == object or p.ndim != 2 or p.shape[1] != 2 * L:
        raise ValueError(f"{what} must be rows of {2 * L} letters")
    if p.size and not np.issubdtype(p.dtype, np.integer):
        raise ValueError(f"{what} must hold integer letters")
    p = np.ascontiguousarray(p, dtype=np.int32)
    if np.any(np.abs(p) > 2):
        raise ValueError("acx presentations use letters +-1 (x) and +-2 (y) only")
    for h in (p[:, :L], p[:, L:]):
        nz = h != 0
        n = nz.sum(1)
        bad = (n == 0) | (nz != (np.arange(L)[None, :] < n[:, None])).any(1)
        if bad.any():
            i = int(np.nonzero(bad)[0][0])
            raise ValueError(f"{p[i]} is not a valid presentation (row {i})")
    return p


class SolutionCache:
    """A device-resident solution cache for presentations of one max_relator_length L on one device:
    the reference's `solution_cache` dict (state tuple -> list of (action, total_length)) with its
    states on the GPU.  It persists across calls and grows as it is filled.

    Pass it as solution_cache= to value_guided_greedy_search[_many] and mcts_search[_many].  A batch
    sees the cache as it was when the call began -- the reference's loop mutates its dict between two
    searches, a batched call cannot -- so one round of the reference's experiment loop is

        res, st = ..._many(P, scorer, solution_cache=c, return_stats=True)
        solved = [i for i, r in enumerate(res) if r[0]]
        c.backfill_many(P[solved], [res[i][1] for i in solved])

    to_dict() returns the reference's dict exactly, which path won a state included."""

    def __init__(self, L: int, device=None, capacity: int = DEFAULT_CAPACITY):
        if not isinstance(L, (int, np.integer)) or not 1 <= L <= _lib.MAX_L:
            raise ValueError(f"L must be an integer in [1, {_lib.MAX_L}], not {L!r}")
        if not isinstance(capacity, (int, np.integer)) or not 1 <= capacity <= 1 << 33:
            raise ValueError(f"capacity must be an integer in [1, 2^33], not {capacity!r}")
        self.L = int(L)
        self._capacity0 = int(capacity)
        self._device_arg = device
        self._h = None
        self.device = None
        self._paths = []  # ordinal -> the path, verbatim
        self._filled = set()  # (presentation, actions, flags) of the backfills done: a repeat adds nothing

    # -- the handle ---------------------------------------------------------------------------
    def _handle(self):
        if self._h is None:
            lib = _lib.load()
            self.device = _batch_bfs._device(self._device_arg)
            with torch.cuda.device(self.device):
                h = lib.acx_cache_create(self.L, self._capacity0)
            if not h:
                raise _lib.ACXError(f"acx_cache_create(L={self.L}, capacity={self._capacity0}) failed (device memory?)")
            self._h = h
        return self._h

    def attach_to(self, dev):
        """the handle, for a search on device `dev` to attach"""
        h = self._handle()
        if self.device != dev:
            raise ValueError(f"solution_cache lives on {self.device}, the search runs on {dev}")
        return h

    def close(self) -> None:
        """Free the device memory; the cache is empty afterwards."""
        if self._h is not None:
            _lib.load().acx_cache_destroy(self._h)
            self._h = None
        self._paths = []
        self._filled = set()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _info(self):
        out = np.zeros(5, np.int64)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().acx_cache_info(self._handle(), out.ctypes.data, self._stream()), "acx_cache_info")
        if out[4]:
            raise _lib.ACXError("acx_cache: an insert found the table full")
        return dict(entries=int(out[0]), rows=int(out[1]), capacity=int(out[2]), buckets=int(out[3]))

    def __len__(self) -> int:
        return 0 if self._h is None else self._info()["entries"]

    @property
    def capacity(self) -> int:
        """rows the device arrays hold now (acx_cache_bytes(L, capacity) bytes)"""
        return self._capacity0 if self._h is None else self._info()["capacity"]

    def nbytes(self) -> int:
        return cache_bytes(self.L, self.capacity)

    # -- filling ------------------------------------------------------------------------------
    def _fill(self, states, paths, cyclical, expand, replay, name):
        lib, h = _lib.load(), self._handle()
        P = len(states)
        if P == 0:
            return
        lens = np.array([len(p) for p in paths], np.int64)
        poff = np.zeros(P + 1, np.int64)
        np.cumsum(lens, out=poff[1:])
        acts = np.zeros(max(int(poff[-1]), 1), np.int32)
        if replay and poff[-1]:
            acts[:poff[-1]] = np.fromiter((int(m[0]) for p in paths for m in p), np.int64, int(poff[-1]))
        dev = self.device
        with torch.cuda.device(dev):
            stream = self._stream()
            st_d, poff_d, acts_d = (torch.from_numpy(x).to(dev) for x in (states, poff, acts))
            counts = torch.zeros(P, dtype=torch.int64, device=dev)
            err = torch.zeros(P, dtype=torch.int32, device=dev)
            _lib.check(lib.acx_cache_count(h, st_d.data_ptr(), poff_d.data_ptr(), acts_d.data_ptr(), P, cyclical, expand,
                                           replay, counts.data_ptr(), err.data_ptr(), stream), "acx_cache_count")
            err_h = err.cpu().numpy()
            if err_h.any():  # nothing has been written yet
                rows = np.nonzero(err_h)[0].tolist()
                raise AssertionError(f"{name}: a move produced an invalid presentation (utils.py:264-266) while "
                                     f"replaying the paths of rows {rows} (at steps {(err_h[rows] - 1).tolist()})")
            voff = torch.zeros(P + 1, dtype=torch.int64, device=dev)
            torch.cumsum(counts, 0, out=voff[1:])
            total = int(voff[-1].item())
            info = self._info()
            _lib.check(lib.acx_cache_reserve(h, info["rows"] + total, stream), "acx_cache_reserve")
            _lib.check(lib.acx_cache_fill(h, st_d.data_ptr(), poff_d.data_ptr(), acts_d.data_ptr(), voff.data_ptr(),
                                          total, len(self._paths), P, cyclical, expand, replay, stream),
                       "acx_cache_fill")
            torch.cuda.current_stream(dev).synchronize()  # the staging tensors are released after the fill
        self._paths.extend(paths)

    def backfill_many(self, presentations, paths, cyclically_reduce=False, expand_rotations=True) -> "SolutionCache":
        """backfill_solution_cache(cache, presentations[i], paths[i], cyclically_reduce,
        expand_rotations) for every i in order (value_guided_search.py:212-250), in a few launches:
        every path is replayed on the device, and every state before its last -- with
        expand_rotations every rotation of either relator too -- becomes an entry unless the state
        is already one.  The first insertion in the reference's sequential order wins, within the
        call and against earlier calls.

        paths[i]: a list of (action, total_length); the tuples are kept verbatim.
        A path whose replay raises in the reference makes the call raise AssertionError naming the
        rows, and the cache is left unchanged.  This differs from the reference, whose dict keeps
        what it had filled in before the raising move.

        A pair (presentation, actions) that an earlier call backfilled with the same flags is
        skipped: all its states are held.  Every other path costs a store row per state and
        rotation, new or not (capacity doubles as needed, acx_cache_bytes), so the store grows with
        the number of distinct paths handed over, not with the number of entries."""
        states = _rows_2d(presentations, self.L, "presentations")
        paths = [list(p) for p in paths]
        if len(paths) != len(states):
            raise ValueError(f"{len(states)} presentations but {len(paths)} paths")
        for i, p in enumerate(paths):
            if len(p) >= MAX_STEPS:
                raise ValueError(f"path {i} has {len(p)} steps; at most {MAX_STEPS - 1} are supported")
            for m in p:
                if not isinstance(m, (tuple, list)) or len(m) != 2:
                    raise ValueError(f"path {i} must hold (action, total_length) pairs")
        # A (presentation, actions) pair that was backfilled with the same flags before holds every one
        # of its states already, so it would only spend store rows: the round of the class's docstring
        # hands the same solved rows over after every call, and they are dropped here.  (Equal actions
        # replay to equal states; the first one's tuples are the values, as in the reference.)
        cyc, exp = int(bool(cyclically_reduce)), int(bool(expand_rotations))
        keep, keys = [], set()
        for i, p in enumerate(paths):
            try:
                key = (states[i].tobytes(), tuple(int(m[0]) for m in p), cyc, exp)
            except (TypeError, ValueError) as e:
                raise ValueError(f"path {i} must hold (action, total_length) pairs with integer actions") from e
            if key not in self._filled and key not in keys:
                keep.append(i)
                keys.add(key)
        if keep:
            self._fill(states[keep], [paths[i] for i in keep], cyc, exp, 1, "backfill_many")
            self._filled.update(keys)
        return self

    @classmethod
    def from_dict(cls, d, L: int, device=None) -> "SolutionCache":
        """The reference's own dict -- state tuple -> list of (action, total_length) -- uploaded: its
        keys are the entries and its values are kept verbatim (nothing is replayed, so any dict the
        reference accepts is accepted)."""
        if not isinstance(d, dict):
            raise ValueError("from_dict takes a dict")
        c = cls(L, device, capacity=max(DEFAULT_CAPACITY, len(d)))
        if d:
            states = _rows_2d([list(k) for k in d], c.L, "the dict's keys")
            c._fill(states, [list(v) for v in d.values()], 0, 0, 0, "from_dict")
        return c

    # -- reading ------------------------------------------------------------------------------
    def _rows(self, entries: np.ndarray):
        """(keys (M, kw) uint64, meta (M) uint64) of the rows `entries`"""
        M, kw = len(entries), _lib.key_words(self.L)
        if M == 0:
            return np.zeros((0, kw), np.uint64), np.zeros(0, np.uint64)
        lib, h, dev = _lib.load(), self._handle(), self.device
        with torch.cuda.device(dev):
            e_d = torch.from_numpy(np.ascontiguousarray(entries, dtype=np.int64)).to(dev)
            keys = torch.empty((M, kw), dtype=torch.int64, device=dev)
            meta = torch.empty(M, dtype=torch.int64, device=dev)
            _lib.check(lib.acx_cache_rows(h, e_d.data_ptr(), M, keys.data_ptr(), meta.data_ptr(), self._stream()),
                       "acx_cache_rows")
            return keys.cpu().numpy().view(np.uint64), meta.cpu().numpy().view(np.uint64)

    def _values(self, states: np.ndarray, meta: np.ndarray):
        """the dict values of the entries whose states (int8 rows) and meta words are given"""
        L, out = self.L, []
        for s, m in zip(states, meta.tolist()):
            ordinal, step, rel, k = m >> 32, (m >> 9) & (MAX_STEPS - 1), (m >> 8) & 1, m & 0xFF
            value = list(self._paths[ordinal][step:])
            if k:  # reversed(undo_moves): the letters the rotation moved to the relator's end, last first
                nz = s[rel * L:(rel + 1) * L]
                nz = nz[nz != 0]
                total = int(np.count_nonzero(s))
                value = [(CONJ_MOVE[(rel, int(nz[len(nz) - 1 - j]))], total) for j in range(k)] + value
            out.append(value)
        return out

    def tails(self, entries, rels, ks):
        """what follows the state that hit, for hits (entry, rel, k) as lookup() and the engines
        report them: the rotation moves from that state to the entry's, then the entry's value
        (value_guided_search.py:135-151)"""
        entries = np.asarray(entries, np.int64)
        keys, meta = self._rows(entries)
        states = unpack_keys(keys, self.L)
        values = self._values(states, meta)
        L, out = self.L, []
        for s, rel, k, value in zip(states, np.asarray(rels).tolist(), np.asarray(ks).tolist(), values):
            if k:  # the hit state's first k letters are the last k of the entry's rotated relator
                nz = s[rel * L:(rel + 1) * L]
                nz = nz[nz != 0]
                total = int(np.count_nonzero(s))
                value = [(CONJ_MOVE[(rel, -int(nz[len(nz) - k + j]))], total) for j in range(k)] + value
            out.append(value)
        return out

    def lookup(self, states):
        """_check_cache_with_rotations' search for each row of `states` ((N, 2L)): three (N) arrays
        -- entry (int64; -1: neither the state nor a rotation of one relator is cached), rel and k
        (int32): the hit is the state with relator `rel` rotated left by k letters (0, 0: itself)."""
        p = _rows_2d(states, self.L, "states")
        N = len(p)
        if N == 0 or self._h is None:
            return np.full(N, -1, np.int64), np.zeros(N, np.int32), np.zeros(N, np.int32)
        lib, h, dev = _lib.load(), self._handle(), self.device
        with torch.cuda.device(dev):
            st = torch.from_numpy(p).to(dev)
            entry = torch.empty(N, dtype=torch.int64, device=dev)
            rel = torch.empty(N, dtype=torch.int32, device=dev)
            k = torch.empty(N, dtype=torch.int32, device=dev)
            _lib.check(lib.acx_cache_lookup(h, st.data_ptr(), N, entry.data_ptr(), rel.data_ptr(), k.data_ptr(),
                                            self._stream()), "acx_cache_lookup")
            return entry.cpu().numpy(), rel.cpu().numpy(), k.cpu().numpy()

    def paths_for(self, states):
        """_check_cache_with_rotations(state, L, cache) for each row: the path to the trivial state,
        or None."""
        entry, rel, k = self.lookup(states)
        hit = np.nonzero(entry >= 0)[0]
        out = [None] * len(entry)
        for i, t in zip(hit.tolist(), self.tails(entry[hit], rel[hit], k[hit])):
            out[i] = t
        return out

    def to_dict(self) -> dict:
        """The reference's dict: every cached state (a tuple of 2L ints) -> its path."""
        if self._h is None:
            return {}
        lib, h, dev = _lib.load(), self._handle(), self.device
        info = self._info()
        n = info["entries"]
        with torch.cuda.device(dev):
            out = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
            cnt = torch.zeros(1, dtype=torch.int64, device=dev)
            _lib.check(lib.acx_cache_entries(h, out.data_ptr(), n, cnt.data_ptr(), self._stream()), "acx_cache_entries")
            if int(cnt.item()) != n:
                raise _lib.ACXError(f"acx_cache: {int(cnt.item())} table entries for {n} counted states")
            entries = np.sort(out[:n].cpu().numpy())
        keys, meta = self._rows(entries)
        states = unpack_keys(keys, self.L)
        return {tuple(int(v) for v in s): val for s, val in zip(states, self._values(states, meta))}


def check(solution_cache, L):
    """the first check of a search's solution_cache= argument, before any GPU call: ValueError for
    anything that is neither None, a SolutionCache of this L nor a dict"""
    if solution_cache is None or isinstance(solution_cache, dict):
        return
    if not isinstance(solution_cache, SolutionCache):
        raise ValueError("solution_cache must be None, an acx.SolutionCache or a dict, not "
                         f"{type(solution_cache).__name__}")
    if solution_cache.L != L:
        raise ValueError(f"solution_cache is for max_relator_length {solution_cache.L}, the presentations have {L}")


def resolve(solution_cache, L, device):
    """a checked solution_cache= argument -> (SolutionCache or None, whether it is the call's own
    to close): a dict is uploaded for the call and never mutated"""
    if isinstance(solution_cache, dict):
        return SolutionCache.from_dict(solution_cache, L, device), True
    return solution_cache, False
