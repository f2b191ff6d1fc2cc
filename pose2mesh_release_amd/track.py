"""People across video frames on the GPU: which person of this frame is which person of the frames before - csrc/track.hip,
include/p2m.h "Tracking people across frames".  The joint between the crowd front end, whose list order changes from frame to
frame, and the streaming filter video.OneEuroFilter, whose row b must be the same person in every call.

  trk = PoseTracker(slots=16)                          pose_thr=0.1, gate=0.3, min_common=3, max_missed=10
  out = trk(people)                                    people [S, P, Jo, 3] (x, y, conf), one frame of S streams -> out.joints
                                                       [S, T, Jo, 3], out.uid, out.flags, out.fresh, ...; [F, S, P, Jo, 3]: F
                                                       frames per stream in one launch -> [F, S, T, ...]
  col = identity_colours(out.uid, table)               one colour per identity in every frame

people is what crowd.CrowdFilter returns in .joints: NaN slots are nobody.  A track slot that shows a person this frame holds
that person's joints; every other slot is NaN, which the modules behind understand as "nobody" (crowd.py), so neither the
number of people nor who is who ever visits the host.  Each call is one kernel launch, and two elementwise ops for the boolean
views, that allocate and synchronise nothing once the buffers exist; a stream's result depends on that stream alone and is bitwise reproducible.  The default thresholds are
this project's choice, not measured optima.  There is no CPU fallback: CPU tensors raise P2MError.
"""
import ctypes as _ct
import types as _types

import torch

from . import _lib

MAX_PEOPLE = MAX_SLOTS = MAX_JOINTS = 64
FLAG_ALIVE, FLAG_PRESENT, FLAG_BORN, FLAG_FRESH, FLAG_RETIRED = 1, 2, 4, 8, 16
SLOT_ABSENT, SLOT_DROPPED = -1, -2


def _p(t):
    return None if t is None else _ct.c_void_p(t.data_ptr())


def _stream():
    return _ct.c_void_p(torch.cuda.current_stream().cuda_stream)


class PoseTracker:
    """trk = PoseTracker(slots=16, pose_thr=0.1, gate=0.3, min_common=3, max_missed=10)
    out = trk(people fp32 [S, P, Jo, 3] | [F, S, P, Jo, 3])
    trk.reset();  trk.reset(mask)

    people: (x, y, confidence) of up to P <= 64 people per frame in any order, a slot with a NaN or an infinity is nobody.
    T = slots <= 64 tracks per stream.  A person is matched to the alive track whose stored pose is nearest - the mean
    |difference| over the coordinates of the joints valid (conf > pose_thr) in both, at least min_common of them, divided by
    the track's extent (the larger side of the box of its valid joints, at least 1) - if that cost is below gate; pairs are
    taken greedily in globally ascending cost.  Unmatched people are born into the lowest slots that were free when the frame
    began and get a fresh uid; people beyond the free slots are dropped.  A track without a detection for more than max_missed
    frames is retired, its slot free from the next frame on (include/p2m.h has the exact arithmetic, all float64).
    The first call creates the state, which fixes S, Jo and the device: trk.pose [S, T, Jo, 3], trk.uid [S, T] (-1 free),
    trk.missed [S, T], trk.next_uid [S].  reset() frees every slot, reset(mask) those of the streams where the bool CUDA tensor
    mask [S] is set: device-side fills; next_uid is kept, so an id is never used twice.
    Returns a namespace of device tensors, buffers kept per input shape and overwritten by the next call of that shape (no
    allocation after the first call of a shape, no sync); [S, ...] for a 4-D input, [F, S, ...] for a 5-D one:
      joints [.., T, Jo, 3]  the slot's person this frame, NaN otherwise
      slot_of [.., P] int32 (-1 absent, -2 dropped), person_of [.., T] int32 (-1 none), uid [.., T] int32 after the frame,
      flags [.., T] uint8 (FLAG_*), cost [.., T] float64 (the matched pair's; NaN for a born or empty slot), dropped [..] int32
      alive, present, born, fresh, retired [.., T] bool: the bits of flags (fresh = has a person and was born or had missed
      frames: what OneEuroFilter.reset(mask=) takes)"""

    def __init__(self, slots=16, pose_thr=0.1, gate=0.3, min_common=3, max_missed=10):
        self.slots = int(slots)
        self.pose_thr, self.gate = float(pose_thr), float(gate)
        self.min_common, self.max_missed = int(min_common), int(max_missed)
        self.pose = self.uid = self.missed = self.next_uid = None
        self._bufs = {}

    def _state(self, S, Jo, dev):
        T = max(self.slots, 0)
        self.pose = torch.zeros((S, T, Jo, 3), device=dev)
        self.uid = torch.full((S, T), -1, device=dev, dtype=torch.int32)
        self.missed = torch.zeros((S, T), device=dev, dtype=torch.int32)
        self.next_uid = torch.zeros((S,), device=dev, dtype=torch.int32)

    @torch.no_grad()
    def __call__(self, people):
        if not isinstance(people, torch.Tensor) or not people.is_cuda:
            raise _lib.P2MError("people: the tracker needs a CUDA tensor (there is no CPU path)")
        if people.dim() not in (4, 5) or people.shape[-1] != 3:
            raise ValueError(f"people: expected [S, P, Jo, 3] or [F, S, P, Jo, 3], got {list(people.shape)}")
        lead = tuple(int(v) for v in people.shape[:-3])
        F, S = (1, lead[0]) if len(lead) == 1 else lead
        P, Jo, dev, T = int(people.shape[-3]), int(people.shape[-2]), people.device, self.slots
        if self.pose is not None and ((S, Jo) != (self.pose.shape[0], self.pose.shape[2]) or dev != self.pose.device):
            raise ValueError(f"people: this tracker follows {self.pose.shape[0]} streams of {self.pose.shape[2]} joints on "
                             f"{self.pose.device}, got {S} of {Jo} on {dev}")
        d = people.contiguous() if people.dtype == torch.float32 else people.to(torch.float32).contiguous()
        key = (lead, P)
        buf = self._bufs.get(key)
        fresh_state = self.pose is None
        if buf is None:
            Tn = max(T, 0)
            bits = torch.zeros((5,) + lead + (Tn,), device=dev, dtype=torch.bool)       # the five views, one ne() per call
            buf = _types.SimpleNamespace(
                joints=torch.full(lead + (Tn, Jo, 3), float("nan"), device=dev),
                slot_of=torch.full(lead + (P,), -1, device=dev, dtype=torch.int32),
                person_of=torch.full(lead + (Tn,), -1, device=dev, dtype=torch.int32),
                uid=torch.full(lead + (Tn,), -1, device=dev, dtype=torch.int32),
                flags=torch.zeros(lead + (Tn,), device=dev, dtype=torch.uint8),
                cost=torch.full(lead + (Tn,), float("nan"), device=dev, dtype=torch.float64),
                dropped=torch.zeros(lead, device=dev, dtype=torch.int32),
                alive=bits[0], present=bits[1], born=bits[2], fresh=bits[3], retired=bits[4])
            buf._bits, buf._masked = bits, torch.zeros_like(bits, dtype=torch.uint8)
            buf._which = torch.tensor([FLAG_ALIVE, FLAG_PRESENT, FLAG_BORN, FLAG_FRESH, FLAG_RETIRED], dtype=torch.uint8
                                      ).to(dev).reshape((5,) + (1,) * (len(lead) + 1))
        if fresh_state:
            self._state(S, Jo, dev)
        try:
            with torch.cuda.device(dev):
                _lib.check(_lib.hip().p2m_pose_track(
                    _p(d), F, S, P, T, Jo, self.pose_thr, self.gate, self.min_common, self.max_missed, _p(self.pose),
                    _p(self.uid), _p(self.missed), _p(self.next_uid), _p(buf.joints), _p(buf.slot_of), _p(buf.person_of),
                    _p(buf.uid), _p(buf.flags), _p(buf.cost), _p(buf.dropped), _stream()), "p2m_pose_track")
        except _lib.P2MError:
            if fresh_state:                                 # (a refused first call fixes nothing)
                self.pose = self.uid = self.missed = self.next_uid = None
            raise
        torch.bitwise_and(buf.flags[None], buf._which, out=buf._masked)
        torch.ne(buf._masked, 0, out=buf._bits)
        self._bufs[key] = buf                               # (kept only once the arguments have passed)
        return buf

    @torch.no_grad()
    def reset(self, mask=None):
        """Frees every slot, or those of the streams where mask (bool [S], on the device) is set.  Ids go on counting."""
        if self.pose is None:
            return
        if mask is None:
            self.uid.fill_(-1)
            self.missed.zero_()
            return
        if not isinstance(mask, torch.Tensor) or not mask.is_cuda:
            raise _lib.P2MError("mask: the tracker needs a CUDA tensor (there is no CPU path)")
        if mask.dtype != torch.bool or tuple(mask.shape) != (self.uid.shape[0],) or mask.device != self.uid.device:
            raise ValueError(f"mask: expected a bool tensor [{self.uid.shape[0]}] on {self.uid.device}")
        self.uid.masked_fill_(mask[:, None], -1)
        self.missed.masked_fill_(mask[:, None], 0)


def identity_colours(uid, table):
    """table[uid.clamp_min(0) % len(table)]: one colour per identity.  uid: PoseTracker's out.uid (any shape); table [n, C]:
    e.g. crowd.person_colours(n).rgb (MeshRenderer's colours) or .u8 (PoseOverlay's), drawn ONCE for the video.  A gather with
    plain torch ops: it allocates its result (inside a captured graph, from the graph's pool).  The rows of free slots
    (uid = -1) take colour 0, which is harmless: those slots show nobody."""
    return table[uid.clamp_min(0).long() % table.shape[0]]
