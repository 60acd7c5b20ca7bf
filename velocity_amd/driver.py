"""Device-resident counterpart of the reference's frame loop (vidExample.py:75-171): TrackerSession keeps the track
state of `batch` video streams on the GPU and advances all of them one frame per step() through vh_session_step.
Inputs are torch CUDA uint8 frames (dense, H x W; a stream's frame size and intrinsics are its own, up to the session's
maximum); results (P, B, S, masks, points) are read back on demand."""
import ctypes as C
import dataclasses
import functools
import math
import typing

import numpy as np

from . import _lib as L


class TrackerSession:
    def __init__(self, K, width, height, n0, nhist=20, batch=1, lk_coarse=None, lk_fine=None, msv_frame=5, fallback=False, fallback_params=None,
                 replenish=None, spare=0, replenish_settings=None, refine_robust=None):
        """width x height: the LARGEST frame a slot can hold; K: the camera a slot has until init_stream / admit gives it another (vh_session_set_camera).
        fallback=True (default off: a step queues exactly what it always did): the recovery branch of KLTmain (KLT.py:130-133) for a stream whose coarse
        stage fails -- the affine from feature matching (vh_match_affine_batch over the failed streams; `fallback_params`: _lib.MATCH_DEFAULTS keys)
        drives the fine stage.  It costs ONE host read per step (the failure flags), so the host no longer runs ahead of the device, and such a step cannot
        be captured into a graph: leave it off for clips that do not need it (include/velocity_hip.h, vh_session_set_fallback).
        spare: rows behind the n0 a slot's frame 0 may fill -- the session has n0 + spare rows (self.n0), and a slot's clip may start with fewer tracks
        than rows (init_stream with fewer points, admit with settings.cap below the rows).  replenish: None (default: a step queues exactly what it always
        did), or a Replenish: lost tracks are replaced by new corners in the spare rows and triangulated on the device (vh_session_set_replenish);
        replenish_settings: the Frame0Settings whose detector and sub-pixel settings the births use (default: the reference's).  state() then gains
        born, tri and n_rows.  refine_robust: None, or the Huber threshold in pixels of every refinement (set_refine_robust)."""
        torch = L.torch_cuda()
        self.torch = torch
        self.spare = int(spare)
        if self.spare < 0:
            raise ValueError(f"spare must be at least 0, got {spare}")
        n0 = int(n0) + self.spare
        self.batch, self.w, self.h, self.n0, self.nhist = batch, width, height, n0, nhist
        self.ws = L.Workspace(batch, width, height, n0)
        self.lib = self.ws.lib
        self.K64 = L.host_K(K)
        k_is_f32 = L.k_is_float32(K)  # numpy builds fcnMSV1_t's rays in float32 then (utils/MSV.py:15-17)
        self._cam0 = (width, height, self.K64.tobytes(), k_is_f32)
        self._cam = [self._cam0] * batch  # host mirror of every slot's camera: (w, h, K bytes, K is float32)
        self.lkc = L.lk_params(dict(L.LK_COARSE, **(lk_coarse or {})))
        self.lkf = L.lk_params(dict(L.LK_FINE, **(lk_fine or {})))
        h = C.c_void_p()
        L.check(self.lib.vh_session_create(C.byref(h), self.ws.handle, n0, nhist, width, height, self.K64.ctypes.data_as(L.f64p), k_is_f32,
                                           C.byref(self.lkc), C.byref(self.lkf), int(msv_frame)), "vh_session_create")
        self.handle = h
        self.fallback = bool(fallback)
        if self.fallback:
            mp = L.match_params(fallback_params)
            L.check(self.lib.vh_session_set_fallback(h, 1, C.byref(mp)), "vh_session_set_fallback")
        self.replenish = replenish
        if replenish is not None:
            rp = L.replenish_params(replenish, replenish_settings or Frame0Settings())
            L.check(self.lib.vh_session_set_replenish(h, C.byref(rp), L.stream_ptr()), "vh_session_set_replenish")
        self._frames = torch.zeros(batch, dtype=torch.int64, device="cuda")  # device table of frame pointers
        # the lifetime rule of a slot: its current frame (the im0 of its next step) and the device inputs of its initialisation (read by a kernel that may
        # not have run yet) stay alive until the slot is initialised again -- by init_stream or by admit, which both replace the slot's entries here
        self._keep = [None] * batch
        self._init_keep = [None] * batch
        self._frame_i = [0] * batch  # host mirror of every slot's frame counter (refine: a clip is finished when it has had all its frames)
        self.refine_robust = 0.0
        if refine_robust is not None:
            self.set_refine_robust(refine_robust)

    def set_refine_robust(self, delta):
        """Huber weights for every refinement of this session from now on (vh_session_set_refine_robust): delta pixels, finite and >= 0; 0 (the default)
        turns them off.  refine() and refine_windows() (with or without min_obs) then weight a measurement whose reprojection error |r| exceeds delta by
        delta / |r|, in every iteration, and their dicts gain robust, nout_first and nout_last: the threshold and how many measurements were
        down-weighted at the first and at the last iteration run.  A host setting: nothing is queued.  The records grow by 16 bytes while it is on, so
        the layouts are kept per setting."""
        L.check(self.lib.vh_session_set_refine_robust(self.handle, float(delta)), "vh_session_set_refine_robust")
        self.refine_robust = float(delta)

    def slot_size(self, slot):
        """(H, W) of the frames slot `slot` takes."""
        return self._cam[slot][1], self._cam[slot][0]

    def _set_camera(self, slot, w, h, K):
        """The slot's frame size and intrinsics (K None: the session's) for its next initialisation: vh_session_set_camera, stream-ordered, and only when
        they differ from what the slot has -- a session of one camera never makes the call."""
        cam = self._cam0[2:] if K is None else (L.host_K(K).tobytes(), L.k_is_float32(K))
        cam = (int(w), int(h)) + cam
        if cam != self._cam[slot]:
            K64 = np.frombuffer(cam[2], np.float64)
            L.check(self.lib.vh_session_set_camera(self.handle, slot, cam[0], cam[1], K64.ctypes.data_as(L.f64p), cam[3], L.stream_ptr()), "vh_session_set_camera")
            self._cam[slot] = cam

    def init_stream(self, slot, frame0, p, p3, vp, t0, time0=0.0, frame_no=0.0, res0=0.0, K=None):
        """Frame-0 state (vidExample.py:116-131): points p [n,2], world points p3 [n,3], pose mask vp, plate pose t0; n = the session's rows, or fewer:
        the rows behind them are tracks that never existed (spare rows).  numpy arrays or CUDA tensors
        (tensors of the right dtype are used in place: a stream can be re-initialised without touching the host).  The slot takes its frame size from
        frame0.shape (at most the session's) and its intrinsics from K (None: the session's)."""
        torch = self.torch
        f0 = _to_device([frame0])[0]
        assert f0.dim() == 2 and f0.dtype == torch.uint8
        fh, fw = f0.shape
        if fw > self.w or fh > self.h:
            raise ValueError(f"init_stream: slot {slot}: a {fw} x {fh} frame does not fit the session's {self.w} x {self.h}")

        def dev(a, np_dtype, t_dtype):
            return L.to_dev(a if isinstance(a, torch.Tensor) else np.asarray(a).astype(np_dtype), t_dtype)

        pd, p3d, vpd = dev(p, np.float32, torch.float32), dev(p3, np.float64, torch.float64), dev(vp, np.uint8, torch.uint8)
        n = pd.shape[0]
        assert 1 <= n <= self.n0 and pd.shape == (n, 2) and p3d.shape == (n, 3) and vpd.shape == (n,)
        t0 = np.ascontiguousarray(np.asarray(t0, np.float32).reshape(3))
        self._set_camera(slot, fw, fh, K)
        if n < self.n0:  # fewer tracks than rows: the count travels as a device value, like admit's (vh_session_init_dev)
            t0d, r0d, nd = L.to_dev(t0, torch.float32), L.to_dev(np.array([res0], np.float64), torch.float64), L.to_dev(np.array([n], np.int32), torch.int32)
            L.check(self.lib.vh_session_init_dev(self.handle, slot, L.dptr(f0), fw, L.dptr(pd), L.dptr(p3d), L.dptr(vpd), L.dptr(t0d), L.dptr(r0d), L.dptr(nd),
                                                 float(time0), float(frame_no), L.stream_ptr()), "vh_session_init_dev")
            self._keep[slot], self._init_keep[slot], self._frame_i[slot] = f0, (pd, p3d, vpd, t0d, r0d, nd), 0
            return
        L.check(self.lib.vh_session_init(self.handle, slot, L.dptr(f0), fw, L.dptr(pd), L.dptr(p3d), L.dptr(vpd), t0.ctypes.data_as(L.f32p),
                                         float(time0), float(frame_no), float(res0), L.stream_ptr()), "vh_session_init")
        self._keep[slot], self._init_keep[slot], self._frame_i[slot] = f0, (pd, p3d, vpd), 0

    def admit(self, entries, settings, anchor=None):
        """THE admission (vidExample.py:105-131 for each clip): frame 0 of every entry computed and installed on the device, on the current stream.
        entries = [(slot, frame0, q, time0, frame_no0[, K]), ...]: frame0 a dense CUDA uint8 [H, W] tensor (the slot takes its size: at most the
        session's), q the clicked plate corners [4, 2], K the clip's intrinsics (absent / None: the session's); settings: a Frame0Settings whose .cap
        is this session's track capacity.  ONE frame-0 batch call for all entries, in the given order (vh_frame0_init_batch3 when their cameras differ
        from the session's), then per entry vh_session_set_camera (only for a slot whose camera changes) and one vh_session_init_dev, fed by the batch's device outputs (count included: nothing is read back).  The session keeps each slot's frame
        and its rows of those outputs alive until the slot is initialised again.  Returns one Admitted per entry: the frame-0 facts a result needs and
        the stream's state does not hold.  anchor="plate": every admitted clip's tracks 0..3 -- the plate corners, whose frame-0 coordinates come from the
        plate's known size -- become the anchors of its slot (set_anchors as a snapshot, right behind the initialisation)."""
        assert anchor in (None, "plate"), anchor
        if self.spare or self.replenish is not None:
            assert settings.cap <= self.n0, "the session's rows must hold 4 + max_corners tracks"
        else:
            assert settings.cap == self.n0, "the session's track capacity must be 4 + max_corners"
        assert all(e[1].is_cuda and e[1].dtype == self.torch.uint8 and e[1].dim() == 2 and e[1].is_contiguous() for e in entries)
        Ks = [e[5] if len(e) > 5 else None for e in entries]
        for (slot, f0, *_), _K in zip(entries, Ks):
            if f0.shape[1] > self.w or f0.shape[0] > self.h:
                raise ValueError(f"admit: slot {slot}: a {f0.shape[1]} x {f0.shape[0]} frame does not fit the session's {self.w} x {self.h}")
        bufs = settings.outputs(len(entries))
        if all(K is None and e[1].shape == (self.h, self.w) for e, K in zip(entries, Ks)):  # the session's own camera throughout
            rois = _frame0_batch_call(self.ws, [e[1] for e in entries], [e[2] for e in entries], self.K64, settings, bufs)
        else:
            rois = _frame0_batch3_call(self.ws, [e[1] for e in entries], [e[2] for e in entries], [self.K64 if K is None else K for K in Ks], settings, bufs)
        out = []
        for a, ((slot, f0, _, time0, frame_no0, *_), K) in enumerate(zip(entries, Ks)):
            p, p3, vp, t0, R0, res0, n0 = rows = tuple(x[a:a + 1] for x in bufs)
            self._set_camera(slot, f0.shape[1], f0.shape[0], K)
            L.check(self.lib.vh_session_init_dev(self.handle, slot, L.dptr(f0), f0.shape[1], L.dptr(p), L.dptr(p3), L.dptr(vp), L.dptr(t0), L.dptr(res0), L.dptr(n0),
                                                 float(time0), float(frame_no0), L.stream_ptr()), "vh_session_init_dev")
            self._keep[slot], self._init_keep[slot], self._frame_i[slot] = f0, rows, 0
            if anchor == "plate":
                self.set_anchors(slot, [0, 1, 2, 3])
            out.append(Admitted(tuple(rois[8 * a:8 * a + 4]), tuple(rois[8 * a + 4:8 * a + 8]), R0[0], res0))
        return out

    def set_anchors(self, slot, ids, xyz=None):
        """The anchored points of the slot's clip (vh_session_set_anchors): track ids whose world coordinates are known, which refine() and
        refine_windows() hold fixed -- they pin the scale of the adjustment.  xyz [n, 3] in the coordinates of the clip's camera 0, or None: the slot's
        current p3 rows of those ids, taken on the current stream (take them before the re-triangulation frame, which overwrites p3 of the surviving
        tracks).  ids = []: no anchors.  Initialising the slot again clears them.  Stream-ordered: nothing is uploaded, nothing waits."""
        ids = np.ascontiguousarray(np.asarray(ids, np.int32).reshape(-1))
        xp = None
        if xyz is not None:
            xyz = np.ascontiguousarray(np.asarray(xyz, np.float64))
            if xyz.shape != (len(ids), 3):
                raise ValueError(f"set_anchors: xyz must be [{len(ids)}, 3], got {xyz.shape}")
            xp = xyz.ctypes.data_as(L.f64p)
        L.check(self.lib.vh_session_set_anchors(self.handle, int(slot), ids.ctypes.data_as(L.i32p), len(ids), xp, L.stream_ptr()), "vh_session_set_anchors")

    def anchors(self, slot):
        """(ids int32 [n] ascending, xyz float64 [n, 3]) of the slot's anchors, read back from the device (waits for it: for tests)."""
        ids, xyz = np.zeros(self.n0, np.int32), np.zeros((self.n0, 3), np.float64)
        n = self.lib.vh_session_anchors(self.handle, int(slot), ids.ctypes.data_as(L.i32p), xyz.ctypes.data_as(L.f64p))
        if n < 0:
            L.check(n, "vh_session_anchors")
        return ids[:n].copy(), xyz[:n].copy()

    def set_frames(self, frames):
        """frames: list of `batch` CUDA uint8 [H,W] tensors, each of its slot's size (kept alive until the next call replaces them); a None entry is a stream that sits the step
        out: its table entry is a null pointer and the frame of its last active step stays alive (it is the im0 of its next active one).
        -> None when every stream has a frame, else the host mask uint8 [batch] of the active streams."""
        torch = self.torch
        assert len(frames) == self.batch
        ptrs = []
        for b, f in enumerate(frames):
            if f is None:
                ptrs.append(0)
                continue
            assert f.is_cuda and f.dtype == torch.uint8 and f.shape == self.slot_size(b) and f.is_contiguous()
            ptrs.append(f.data_ptr())
        self._prev_keep = self._keep
        self._keep = [k if f is None else f for f, k in zip(frames, self._keep)]
        self._frames.copy_(torch.tensor(ptrs, dtype=torch.int64), non_blocking=False)
        return None if all(ptrs) else np.array([1 if q else 0 for q in ptrs], np.uint8)

    def step(self, frames=None, time_s=0.0, frame_no=0.0, frames_table=None, active=None):
        """One frame for every stream.  Either `frames` (list of tensors) or `frames_table` (int64 CUDA tensor of pointers).

        A stream may sit the step out (vh_session_step_some): a None entry of `frames`, or with `frames_table` a zero pointer AND a zero in `active`
        (host uint8 [batch]; the two must agree).  Its state is untouched -- a slot that was never initialised is a legal idle stream -- and its last
        frame stays alive until its next active step.  Without idle streams the step takes exactly the calls it always took.

        time_s / frame_no: scalars (every stream shares the clock) or sequences / tensors of `batch` values (independent videos,
        each with its own CAP_PROP_POS_MSEC and frame counter).  With `frames_table` the caller owns the frame buffers: the
        frames of step i are read again by step i+1 (as im0) and must stay alive until that step has run."""
        if frames is not None:
            active = self.set_frames(frames)
        tab = self._frames if frames_table is None else frames_table
        self._frame_i = [i + (1 if active is None or active[b] else 0) for b, i in enumerate(self._frame_i)]
        is_t = [hasattr(x, "is_cuda") for x in (time_s, frame_no)]  # torch tensors first: numpy must never see a CUDA tensor
        if active is None and not any(is_t) and np.ndim(time_s) == 0 and np.ndim(frame_no) == 0:
            L.check(self.lib.vh_session_step(self.handle, L.dptr(tab), float(time_s), float(frame_no), L.stream_ptr()), "vh_session_step")
            return
        torch = self.torch

        def clock(x, tensor):  # scalar / 0-dim / length-batch, host or device -> float32 CUDA vector of `batch` values
            if tensor:
                t = L.to_dev(x, torch.float32).reshape(-1)
                return t.expand(self.batch).contiguous() if t.numel() == 1 else t
            return L.to_dev(np.array(np.broadcast_to(np.asarray(x, np.float32), (self.batch,))), torch.float32)

        tv, fv = clock(time_s, is_t[0]), clock(frame_no, is_t[1])
        assert tv.numel() == self.batch and fv.numel() == self.batch
        self._clock_keep = (tv, fv)
        if active is not None:
            act = np.ascontiguousarray(active, np.uint8)
            assert act.shape == (self.batch,)
            L.check(self.lib.vh_session_step_some(self.handle, L.dptr(tab), act.ctypes.data, L.dptr(tv), L.dptr(fv), L.stream_ptr()), "vh_session_step_some")
            return
        L.check(self.lib.vh_session_step_v(self.handle, L.dptr(tab), L.dptr(tv), L.dptr(fv), L.stream_ptr()), "vh_session_step_v")

    def step_bgr(self, frames_bgr, time_s=0.0, frame_no=0.0):
        """One frame for every stream straight from BGR frames (the decoder's output, vidExample.py:89-91): the fused ingest writes the gray frames
        and the quarter-scale images in one pass (vh_session_ingest_bgr), then the step runs on them.  frames_bgr: list of `batch` CUDA uint8 [H,W,3]
        tensors, each of its slot's size.  The session owns two sets of gray buffers (a frame is read by two steps: as `im`, then as `im0`).
        A None entry is a stream that sits the step out, as in step(): nothing of it is ingested, and its gray frame of its last active step is kept (each
        stream alternates between its two buffers on its own active steps).  Returns the gray frames of the step: the [batch, H, W] buffer, or with idle
        streams -- or with slots of other sizes than the session's -- a list (None for an idle stream, else the slot's [H_b, W_b] gray frame)."""
        torch = self.torch
        assert len(frames_bgr) == self.batch
        if getattr(self, "_gray", None) is None:
            self._gray = [torch.empty((self.batch, self.h, self.w), dtype=torch.uint8, device="cuda") for _ in range(2)]
            self._gray_tab = [torch.tensor([g[b].data_ptr() for b in range(self.batch)], dtype=torch.int64, device="cuda") for g in self._gray]
            self._gray_i = 0
            self._gray_k = [0] * self.batch  # per stream: the buffer its next active step writes
        ptrs = []
        for b, f in enumerate(frames_bgr):
            if f is None:
                ptrs.append(0)
                continue
            assert f.is_cuda and f.dtype == torch.uint8 and f.shape == self.slot_size(b) + (3,) and f.is_contiguous()
            ptrs.append(f.data_ptr())
        sizes = [self.slot_size(b) for b in range(self.batch)]
        mixed = any(sz != (self.h, self.w) for sz in sizes)  # a slot's dense gray frame is the front of its (maximum-sized) buffer
        bgr_stride = 0 if mixed else 3 * self.w  # 0: dense rows of every stream's own width
        self._bgr_keep = list(frames_bgr)
        bgr_tab = torch.tensor(ptrs, dtype=torch.int64).cuda()
        self._bgr_tab_keep = bgr_tab
        if mixed or not all(ptrs) or len(set(self._gray_k)) > 1:  # some stream is idle now, or was: the streams no longer alternate in step
            ks = self._gray_k
            gray = [None if not q else self._gray[ks[b]][b].reshape(-1)[: sizes[b][0] * sizes[b][1]].view(sizes[b]) for b, q in enumerate(ptrs)]
            gtab = torch.tensor([0 if g is None else g.data_ptr() for g in gray], dtype=torch.int64).cuda()
            self._gray_k = [k ^ 1 if q else k for k, q in zip(ks, ptrs)]
            L.check(self.lib.vh_session_ingest_bgr(self.handle, L.dptr(bgr_tab), bgr_stride, L.dptr(gtab), L.stream_ptr()), "vh_session_ingest_bgr")
            self._gray_tab_keep = gtab
            self.step(frames_table=gtab, time_s=time_s, frame_no=frame_no, active=np.array([1 if q else 0 for q in ptrs], np.uint8))
            return gray
        k = self._gray_k[0]
        self._gray_k = [k ^ 1] * self.batch
        self._gray_i = k ^ 1
        L.check(self.lib.vh_session_ingest_bgr(self.handle, L.dptr(bgr_tab), 3 * self.w, L.dptr(self._gray_tab[k]), L.stream_ptr()), "vh_session_ingest_bgr")
        self.step(frames_table=self._gray_tab[k], time_s=time_s, frame_no=frame_no)
        return self._gray[k]

    def recoveries(self):
        """int [batch, 2]: per stream, the steps since its init_stream in which the recovery ran / in which it found a model."""
        out = np.zeros((self.batch, 2), np.int32)
        L.check(self.lib.vh_session_recoveries(self.handle, out.ctypes.data_as(L.i32p)), "vh_session_recoveries")
        return out

    def replenish_state(self, slot=0):
        """(born int32 [N0], tri uint8 [N0], counts int32 [4] = n_rows, rows born, promoted, rejected) of the slot (vh_session_replenish_state: waits for
        the device; for tests and for the results of a finished clip)."""
        born, tri, counts = np.zeros(self.n0, np.int32), np.zeros(self.n0, np.uint8), np.zeros(4, np.int32)
        L.check(self.lib.vh_session_replenish_state(self.handle, int(slot), born.ctypes.data_as(L.i32p), tri.ctypes.data, counts.ctypes.data_as(L.i32p)),
                "vh_session_replenish_state")
        return born, tri, counts

    def view(self, slot=0):
        v = L.SessionView()
        L.check(self.lib.vh_session_ptrs(self.handle, slot, C.byref(v)), "vh_session_ptrs")
        return v

    def _rd(self, ptr, count, dtype):
        out = np.empty(count, dtype)
        if count:
            L.check(self.lib.vh_copy_to_host(out.ctypes.data, ptr, out.nbytes, L.stream_ptr()), "vh_copy_to_host")
        return out

    def lk_launches(self):
        """What the library says the three LK launches of the last step were (the launcher's own decisions): kernel names (vh_profile_lk_routes) and launch
        slots per workgroup (vh_profile_lk_tpw) of stage 0 (quarter scale), 1 (coarse ROI), 2 (fine)."""
        routes, names, tpw = (C.c_int * 3)(), C.create_string_buffer(96), (C.c_int * 3)()
        L.check(self.lib.vh_profile_lk_routes(self.ws.handle, routes, names), "vh_profile_lk_routes")
        L.check(self.lib.vh_profile_lk_tpw(self.ws.handle, tpw), "vh_profile_lk_tpw")
        return dict(kernels=[names.raw[32 * k:32 * k + 32].split(b"\0")[0].decode() for k in range(3)], routes=list(routes), slots_per_workgroup=list(tpw))

    def state(self, slot=0):
        """Host copy of the stream state: dict(vg, vp, p, P, B, S, p3, t, res, n_cur, n_pose, frame_i, klt_flags).
        P comes back in the reference's [5, N0, nhist] layout (the device keeps it frame-major, [nhist, 5, N0]: include/velocity_hip.h).
        With replenish on also born int32 [N0], tri uint8 [N0] and n_rows (replenish_state)."""
        v = self.view(slot)
        n0, nh = self.n0, self.nhist
        n_cur = int(self._rd(v.n_cur, 1, np.int32)[0])
        n_pose = int(self._rd(v.n_pose, 1, np.int32)[0])
        extra = {}
        if self.replenish is not None:
            born, tri, counts = self.replenish_state(slot)
            extra = dict(born=born, tri=tri, n_rows=int(counts[0]))
        return dict(
            **extra,
            vg=self._rd(v.vg, n0, np.uint8).astype(bool), vp=self._rd(v.vp, n0, np.uint8).astype(bool),
            p=self._rd(v.p, 2 * n_cur, np.float32).reshape(n_cur, 2), ids=self._rd(v.ids, n_cur, np.int32),
            P=np.ascontiguousarray(self._rd(v.P, 5 * n0 * nh, np.float32).reshape(nh, 5, n0).transpose(1, 2, 0)), B=self._rd(v.B, nh * 14, np.float32).reshape(nh, 14),
            S=self._rd(v.S, nh * 9, np.float32).reshape(nh, 9), p3=self._rd(v.p3, 3 * n0, np.float64).reshape(n0, 3),
            t=self._rd(v.t, 3, np.float32), res=float(self._rd(v.res, 1, np.float64)[0]), n_cur=n_cur, n_pose=n_pose,
            frame_i=int(self._rd(v.frame_i, 1, np.int32)[0]), klt_flags=int(self._rd(v.klt_flags, 1, np.int32)[0]),
            pose_info=self._rd(v.pose_info, 2, np.int32))

    def record_layout(self):
        """vh_session_record of this session: byte offsets of the fields of an exported record (and `bytes`, its size)."""
        if getattr(self, "_layout", None) is None:
            lay = L.SessionRecord()
            if not self.lib.vh_session_export_size(self.handle, C.byref(lay)):
                L.check(-1, "vh_session_export_size")
            self._layout = lay
        return self._layout

    def export(self, slot=0, out=None):
        """Everything state() returns, without stopping the device: ONE launch packs the stream into a contiguous record (vh_session_export: the history
        is transposed to the reference's [5, N0, nhist] on the device), ONE asynchronous copy brings it into the pinned buffer `out` (uint8 torch tensor
        of record_layout().bytes bytes; a new one if None) and an event marks its arrival.  Returns a handle: .done() polls, .result() waits for the event
        and returns the dict of state() (fresh arrays: `out` may be reused afterwards); .recoveries are the stream's recovery counters (vh_session_recoveries)
        at the time of the call.  Issue it on the session's HIP stream, like every call of the session."""
        torch = self.torch
        lay = self.record_layout()
        if getattr(self, "_rec_dev", None) is None:
            self._rec_dev = torch.empty(lay.bytes, dtype=torch.uint8, device="cuda")  # one per session: packs and copies are ordered by its stream
        if out is None:
            out = torch.empty(lay.bytes, dtype=torch.uint8).pin_memory()
        assert out.dtype == torch.uint8 and out.numel() >= lay.bytes and out.is_pinned() and out.is_contiguous()
        L.check(self.lib.vh_session_export(self.handle, slot, L.dptr(self._rec_dev), L.stream_ptr()), "vh_session_export")
        out[: lay.bytes].copy_(self._rec_dev, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return ExportedState(out, lay, ev, self.recoveries()[slot])

    def refine_layout(self, max_iter=10):
        """vh_refine_record of this session for max_iter iterations: byte offsets of the fields of a refined clip's record (and `bytes`, its size)."""
        lays = self.__dict__.setdefault("_refine_layouts", {})
        key = (int(max_iter), self.refine_robust)  # (the record has a tail while the session refines with Huber weights)
        if key not in lays:
            lay = L.RefineRecord()
            if not self.lib.vh_session_refine_size(self.handle, int(max_iter), C.byref(lay)):
                L.check(-1, "vh_session_refine_size")
            lay.robust = self.refine_robust
            lays[key] = lay
        return lays[key]

    def _refine_request(self, call, items, lay, nf, out, chunk, need):
        """THE refinement request behind refine() and refine_windows(): `items` (slots or windows) go to the library `chunk` at a time -- call(part, recs)
        queues one part with its records at device address `recs`, on a scratch of `need` bytes -- then one asynchronous copy per pinned buffer and an
        event.  The scratch and the device records belong to the session and are reused (the chunks share the scratch: they are ordered by the stream).
        out: None (a new pinned buffer), ONE pinned uint8 tensor for all the records, or a list whose entries are a pinned tensor (one record) or
        (pinned tensor, count): consecutive records, `count` of them into that tensor."""
        torch = self.torch
        nbytes = lay.bytes * len(items)
        if getattr(self, "_refine_ws", None) is None or self._refine_ws.numel() < need:
            self._refine_ws = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda")
        if getattr(self, "_refine_dev", None) is None or self._refine_dev.numel() < nbytes:
            self._refine_dev = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        if out is None:
            out = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        parts = [(out, len(items))] if isinstance(out, torch.Tensor) else [(b, 1) if isinstance(b, torch.Tensor) else (b[0], int(b[1])) for b in out]
        assert sum(k for _, k in parts) == len(items)
        assert all(b.dtype == torch.uint8 and b.numel() >= k * lay.bytes and b.is_pinned() and b.is_contiguous() for b, k in parts)
        for w0 in range(0, len(items), chunk):
            call(items[w0:w0 + chunk], C.c_void_p(self._refine_dev.data_ptr() + w0 * lay.bytes))
        at = 0
        for b, k in parts:
            b[: k * lay.bytes].copy_(self._refine_dev[at:at + k * lay.bytes], non_blocking=True)
            at += k * lay.bytes
        ev = torch.cuda.Event()
        ev.record()
        return Refined(parts, lay, ev, chunk, nf)

    def refine(self, slots, max_iter=10, out=None):
        """Bundle adjustment of the finished clips in `slots` (vidExample.py:157: fcnNLS_batch(K, P[:, :, 0:i], p3, B[0:i, 3:6]), NLS.py:186-250), without
        leaving the device: ONE vh_session_refine -- pack, one BA launch sequence for all the slots (their track counts and cameras may differ), unpack --
        then one asynchronous copy per pinned buffer and an event.  The slots must have had the same number of frames, all of their clips' (clips of other
        lengths: another call).  The session's state is only read: its streams step on as if nothing had happened.  The scratch and the device records
        belong to the session and are reused.  out: None (a new pinned buffer), ONE pinned uint8 tensor for all the records, or one per slot.
        Returns a handle like export()'s: .done() polls, .result() waits and returns one dict per slot (unpack_refine)."""
        slots = [int(b) for b in slots]
        if not slots:
            raise ValueError("refine: no slot given")
        nf = self._frame_i[slots[0]] + 1 if 0 <= slots[0] < self.batch else 0  # (a slot outside the session: the library names it)
        need = int(self.lib.vh_session_refine_workspace(self.handle, len(slots), nf)) if nf >= 2 and len(slots) <= self.batch else 0

        def call(part, recs):
            L.check(self.lib.vh_session_refine(self.handle, (C.c_int * len(part))(*part), len(part), nf, int(max_iter), recs, L.dptr(self._refine_ws),
                                               self._refine_ws.numel(), L.stream_ptr()), "vh_session_refine")

        return self._refine_request(call, slots, self.refine_layout(max_iter), nf, out, len(slots), need)
    def refine_window_layout(self, nf, max_iter=10, with_points=False, partial=False):
        """vh_refine_window_record of this session for windows of nf frames: byte offsets of the fields of a refined window's record (and `bytes`).
        partial: vh_refine_partial_record, the record of a refine_windows(min_obs=...) request (.win: the window record's offsets; then the counts')."""
        lays = self.__dict__.setdefault("_refine_window_layouts", {})
        key = (int(nf), int(max_iter), bool(with_points), bool(partial), self.refine_robust)
        if key not in lays:
            lay, fn = (L.RefinePartialRecord(), "vh_session_refine_windows_partial_size") if partial else (L.RefineWindowRecord(), "vh_session_refine_windows_size")
            if not getattr(self.lib, fn)(self.handle, key[0], key[1], int(key[2]), C.byref(lay)):
                L.check(-1, fn)
            lay.robust = self.refine_robust
            lays[key] = lay
        return lays[key]

    def refine_windows(self, windows, nf, max_iter=10, with_points=False, out=None, workspace_budget=None, min_obs=None, start_reproj=0.0):
        """Bundle adjustment of frame windows of the slots' clips without leaving the device (vh_session_refine_windows): `windows` = [(slot, first), ...],
        each the frames [first, first + nf) of its slot's clip -- fcnNLS_batch(K, P[:, :, first:first+nf], ...) in the coordinates of the window's first
        camera, on the tracks alive through the window.  A slot may appear in many windows and need not be finished (first + nf - 1 <= its frame
        counter); the clips may have any lengths.  The session is only read.  The windows go through ONE BA launch sequence per chunk: the scratch grows
        with the number of windows, so a request is issued in chunks of as many windows as keep it under `workspace_budget` bytes (default
        REFINE_WINDOWS_BUDGET; always at least one window).  The scratch and the device records belong to the session and are reused.
        out: None (a new pinned buffer), ONE pinned uint8 tensor for all the records, or a list of (pinned uint8 tensor, count): consecutive records,
        `count` of them into each tensor.  with_points: the records also carry ids and pw (in the window's coordinates).
        min_obs (default None: the call above, unchanged): 2 <= min_obs <= nf -- a window also takes the tracks observed in at least min_obs of its
        frames that have a world point to start from (vh_session_refine_windows_partial: established by the session or anchored; with start_reproj > 0
        also those whose start, triangulated from their first and last observed frame of the window, reprojects within start_reproj pixels).  A missing
        measurement is no observation to the solve.  The dicts then carry nobs, npart, ntri, nrej as well.
        Returns a handle like refine()'s: .done() polls, .result() waits and returns one dict per window (unpack_refine_window), in the order given."""
        wins = [(int(b), int(f)) for b, f in windows]
        if not wins:
            raise ValueError("refine_windows: no window given")
        nf, max_iter = int(nf), int(max_iter)
        partial = min_obs is not None
        if not partial and start_reproj:
            raise ValueError("refine_windows: start_reproj needs min_obs")
        ws_fn = "vh_session_refine_windows_partial_workspace" if partial else "vh_session_refine_windows_workspace"
        lay = self.refine_window_layout(nf, max_iter, with_points, partial)
        budget = REFINE_WINDOWS_BUDGET if workspace_budget is None else int(workspace_budget)
        one = int(getattr(self.lib, ws_fn)(self.handle, 1, nf))
        if not one:
            L.check(-1, ws_fn)
        chunk = max(1, min(budget // one, REFINE_WINDOWS_MOST, len(wins)))
        if chunk < len(wins):  # several calls: what the library would refuse in a later one is refused here, before the first is queued
            if len(set(wins)) != len(wins):
                raise ValueError("refine_windows: a window is given twice")
            for b, f in wins:
                if not 0 <= b < self.batch or f < 0 or f + nf - 1 > self._frame_i[b]:
                    raise ValueError(f"refine_windows: window (slot {b}, first {f}) of {nf} frames is outside the session's {self.batch} slots or the frames its slot has had")

        def call(part, recs):
            tab = (L.RefineWindow * len(part))(*[L.RefineWindow(b, f) for b, f in part])
            if partial:
                prm = L.RefinePartialParams(int(min_obs), float(start_reproj))
                L.check(self.lib.vh_session_refine_windows_partial(self.handle, tab, len(part), nf, max_iter, int(bool(with_points)), C.byref(prm), recs,
                                                                   L.dptr(self._refine_ws), self._refine_ws.numel(), L.stream_ptr()),
                        "vh_session_refine_windows_partial")
                return
            L.check(self.lib.vh_session_refine_windows(self.handle, tab, len(part), nf, max_iter, int(bool(with_points)), recs, L.dptr(self._refine_ws),
                                                       self._refine_ws.numel(), L.stream_ptr()), "vh_session_refine_windows")

        return self._refine_request(call, wins, lay, nf, out, chunk, int(getattr(self.lib, ws_fn)(self.handle, chunk, nf)))

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.torch.cuda.synchronize()
                self.lib.vh_session_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class ExportedState:
    """A stream's state on its way to the host (TrackerSession.export)."""

    def __init__(self, buf, layout, event, recoveries):
        self.buf, self.layout, self.event, self.recoveries = buf, layout, event, recoveries
        self._res = None

    def done(self):
        """True once the record has arrived (never waits)."""
        return self._res is not None or self.event.query()

    def result(self):
        if self._res is None:
            self.event.synchronize()
            self._res = unpack_record(self.buf.numpy(), self.layout)
        return self._res


class Refined:
    """The records of one TrackerSession.refine or refine_windows request on their way to the host, in the order given.  parts: [(pinned buffer, the
    consecutive records it holds)]; bufs: one view per record; chunk: the slots or windows per library call; nf: the frames of a clip or window."""

    def __init__(self, parts, layout, event, chunk, nf):
        self.parts, self.layout, self.event, self.chunk, self.nf = parts, layout, event, chunk, nf
        nb = layout.bytes
        self.bufs = [b[k * nb:(k + 1) * nb] for b, cnt in parts for k in range(cnt)]
        self._res = None

    def done(self):
        """True once the records have arrived (never waits)."""
        return self._res is not None or self.event.query()

    def result(self):
        if self._res is None:
            self.event.synchronize()
            self._res = [_unpack_refined(b.numpy(), self.layout, self.nf) for b in self.bufs]
        return self._res


RefinedClips = RefinedWindows = Refined


# Device scratch one refine_windows chunk may take, in bytes (the keyword workspace_budget overrides it).  A window's share is its z, x0 and BA workspace
# (vh_session_refine_windows_workspace(s, 1, nf): about 1.3 MB at 1004 tracks and 8 frames), so the default holds several hundred such windows per BA
# launch sequence -- enough to fill the chip -- while a request of thousands of windows of a long clip does not grow the scratch without bound.
REFINE_WINDOWS_BUDGET = 1 << 30
REFINE_WINDOWS_MOST = 65535  # windows of one BA launch sequence (vh_nls_batch_windows)


def _unpack_refined(raw, lay, nf=None):
    """THE reader of a refinement record of either layout (uint8 array `raw`, offsets `lay`): the header words, the first nf of the record's rows of cw, dr
    and speed, the scalars, the trace and -- where the record carries them -- ids and pw; every array is a copy."""
    counts = {}
    if getattr(lay, "robust", 0.0):  # the 16-byte tail of a record refined with Huber weights: nout_first, nout_last, delta (float32), 0
        nbytes = lay.win.bytes if isinstance(lay, L.RefinePartialRecord) else lay.bytes
        first, last = np.frombuffer(raw, np.int32, 2, nbytes - 16)
        counts = dict(robust=float(np.frombuffer(raw, np.float32, 1, nbytes - 8)[0]), nout_first=int(first), nout_last=int(last))
    if isinstance(lay, L.RefinePartialRecord):  # the window record, then the four counts
        counts.update({k: int(np.frombuffer(raw, np.int32, 1, getattr(lay, k))[0]) for k in ("nobs", "npart", "ntri", "nrej")})
        lay = lay.win
    window = isinstance(lay, L.RefineWindowRecord)

    def rd(off, count, dtype):
        return np.frombuffer(raw, dtype, count, off).copy()

    head = {k: int(rd(getattr(lay, k), 1, np.int32)[0]) for k in (("slot", "first") if window else ()) + ("nt", "iterations", "converged", "nfix")}
    rows, nt = lay.nf if window else lay.nhist, head["nt"]
    cw = rd(lay.cw, 3 * rows, np.float64).reshape(rows, 3)
    if window:
        nf = rows
    elif nf is None:
        nf = int(np.isfinite(cw[:, 0]).sum())
    one = {k: float(rd(getattr(lay, k), 1, np.float64)[0]) for k in ("speed_mean", "speed_std", "f_first", "f_last")}
    pts = dict(ids=rd(lay.ids, nt, np.int32), pw=rd(lay.pw, 3 * nt, np.float64).reshape(nt, 3)) if not window or lay.with_points else {}
    return dict(cw=cw[:nf].copy(), dr=rd(lay.dr, nf, np.float64), speed=rd(lay.speed, nf, np.float64),
                trace=rd(lay.trace, 2 * head["iterations"], np.float64).reshape(head["iterations"], 2), **head, **one, **pts, **counts)


def unpack_refine(raw, lay, nf=None):
    """A vh_refine_record (uint8 array `raw`, offsets `lay`) as a dict: nt, nfix (anchored points among the nt), ids [nt], pw [nt, 3], cw [nf, 3], dr [nf],
    speed [nf] (entry 0 NaN), speed_mean, speed_std, iterations, converged, trace [iterations, 2], f_first, f_last; every array is a copy.  nf: the clip's frames (None: the
    rows of cw the record defines)."""
    return _unpack_refined(raw, lay, nf)


def unpack_refine_window(raw, lay):
    """A vh_refine_window_record (uint8 array `raw`, offsets `lay`) as a dict: slot, first, nt, nfix (anchored points among the nt; 0: solved free),
    iterations, converged, cw [nf, 3] (relative to the window's
    first camera), dr [nf], speed [nf] (entry 0 NaN), speed_mean, speed_std, f_first, f_last, trace [iterations, 2] and, when the record carries them,
    ids [nt] and pw [nt, 3] (in the window's coordinates: subtract B[first, 3:6] for the session's); every array is a copy.  A vh_refine_partial_record
    (offsets RefinePartialRecord) gives the same and nobs, npart, ntri, nrej."""
    return _unpack_refined(raw, lay)


def refine_window_starts(n, window, stride=None):
    """The first frames of the windows of `window` frames that cover a clip of n frames: range(0, n - window + 1, stride) plus the end-aligned n - window when
    that is not already last, so every frame is in a window.  1 <= stride <= window - 1 (default window - 1): consecutive windows share at least one
    frame, so every frame-to-frame step i-1 -> i lies inside a window -- with the default exactly one, except where the end-aligned window overlaps."""
    n, window = int(n), int(window)
    stride = window - 1 if stride is None else int(stride)
    if window < 2:
        raise ValueError(f"refine_window_starts: window = {window}: a window needs at least two frames")
    if n < window:
        raise ValueError(f"refine_window_starts: a clip of n = {n} frames is shorter than window = {window}")
    if not 1 <= stride <= window - 1:
        raise ValueError(f"refine_window_starts: stride = {stride} is outside 1 .. window - 1 = {window - 1}")
    starts = list(range(0, n - window + 1, stride))
    if starts[-1] != n - window:
        starts.append(n - window)
    return starts


def merge_window_speeds(n, windows):
    """The speed of a clip of n frames from its refined windows (pure NumPy).  windows: dicts with `first`, `speed` [W] (entry 0 NaN: speed[j] is the
    estimate of the step first+j-1 -> first+j), nt, iterations, converged, f_last (unpack_refine_window's).  speed[i] (i >= 1) is the mean of the
    estimates of the windows that cover step i, cover[i] how many did (a step nobody covers: NaN); speed_mean / speed_std are over speed[1:n]
    (vidExample.py:177).  An average of independent estimates, not one global adjustment.  Also returns the per-window arrays first, nt, nfix (0 where a
    window has no such field), iterations, converged, f_last."""
    n = int(n)
    tot, cover = np.zeros(n), np.zeros(n, np.int64)
    for w in windows:
        sp = np.asarray(w["speed"], np.float64)
        lo = int(w["first"])
        assert lo >= 0 and lo + len(sp) <= n, "merge_window_speeds: a window outside the clip"
        tot[lo + 1:lo + len(sp)] += sp[1:]
        cover[lo + 1:lo + len(sp)] += 1
    speed = np.full(n, np.nan)
    hit = cover > 0
    speed[hit] = tot[hit] / cover[hit]
    return dict(speed=speed, cover=cover, speed_mean=float(speed[1:].mean()), speed_std=float(speed[1:].std()),
                first=np.array([w["first"] for w in windows], np.int64), nt=np.array([w["nt"] for w in windows], np.int64),
                nfix=np.array([w.get("nfix", 0) for w in windows], np.int64),
                iterations=np.array([w["iterations"] for w in windows], np.int64), converged=np.array([w["converged"] for w in windows], np.int64),
                f_last=np.array([w["f_last"] for w in windows], np.float64))


def _merged_ba(n, wins, window, stride):
    """result["ba"] of a clip refined in windows: merge_window_speeds' dict with `window` and `stride`; windows refined with min_obs (their dicts carry
    the counts) add the per-window arrays nobs, npart, ntri, nrej, and windows refined with Huber weights `robust` and the arrays nout_first, nout_last."""
    counts = {k: np.array([w[k] for w in wins], np.int64) for k in ("nobs", "npart", "ntri", "nrej", "nout_first", "nout_last") if wins and k in wins[0]}
    if wins and "robust" in wins[0]:  # refined with Huber weights: the threshold, and the counts per window
        counts["robust"] = wins[0]["robust"]
    return dict(merge_window_speeds(n, wins), window=window, stride=stride, **counts)


def _check_partial(refine, refine_min_obs=None, refine_start_reproj=None):
    """-> None (the option is absent), or (min_obs, start_reproj); raises ValueError by name before anything is queued."""
    if refine_min_obs is None:
        if refine_start_reproj is not None:
            raise ValueError("refine_start_reproj needs refine_min_obs")
        return None
    if refine != "ba":
        raise ValueError("refine_min_obs needs refine='ba'")
    m, r = int(refine_min_obs), 0.0 if refine_start_reproj is None else float(refine_start_reproj)
    if m < 2:
        raise ValueError(f"refine_min_obs = {m}: a track needs at least two observations")
    if not (np.isfinite(r) and r >= 0.0):
        raise ValueError(f"refine_start_reproj = {r}: a finite number of pixels >= 0")
    return m, r


def _refine_finished(ses, clips, win, stride, partial=None):
    """The refinement of the clips of session `ses` that have just ended, for all three drivers.  clips = [(slot, clip length, pinned buffer for the
    clip's records or None: for all of them or for none)]; win, stride: _check_refine's.  The clips of at least `win` frames go through ONE
    refine_windows request -- the windows refine_window_starts gives each, a clip's consecutive -- and the others through one refine per clip length,
    shortest first.  Returns per clip (the handle of its request, the function that turns the handle's result into the clip's "ba" dict).
    partial = _check_partial's (min_obs, start_reproj): every request goes through refine_windows(min_obs=...) -- min_obs cut to the window's frames --
    and a clip that is not windowed is ONE window of its own length (one request per clip length, as whole clips have)."""
    done = [None] * len(clips)
    starts = {i: refine_window_starts(n, win, stride) for i, (_, n, _) in enumerate(clips) if win and n >= win}

    def pkw(nf):
        return {} if partial is None else dict(min_obs=min(partial[0], nf), start_reproj=partial[1])

    if starts:
        rh = ses.refine_windows([(clips[i][0], f) for i, st in starts.items() for f in st], win,
                                out=None if clips[0][2] is None else [(clips[i][2], len(st)) for i, st in starts.items()], **pkw(win))
        at = 0
        for i, st in starts.items():
            done[i] = (rh, lambda r, at=at, k=len(st), n=clips[i][1]: _merged_ba(n, r[at:at + k], win, stride))
            at += len(st)
    for n_clip in sorted({n for i, (_, n, _) in enumerate(clips) if i not in starts}):
        same = [i for i, (_, n, _) in enumerate(clips) if i not in starts and n == n_clip]
        if partial is not None:
            rh = ses.refine_windows([(clips[i][0], 0) for i in same], n_clip, out=None if clips[0][2] is None else [(clips[i][2], 1) for i in same],
                                    **pkw(n_clip))
            for idx, i in enumerate(same):
                done[i] = (rh, lambda r, idx=idx, n=n_clip: _merged_ba(n, r[idx:idx + 1], n, n - 1))
            continue
        rh = ses.refine([clips[i][0] for i in same], out=None if clips[0][2] is None else [clips[i][2] for i in same])
        for idx, i in enumerate(same):
            done[i] = (rh, lambda r, idx=idx: r[idx])
    return done


def ba_line(ba):
    """The line a refined clip adds behind the reference's summary (a clip refined in windows: their count and length, the fewest and the most tracks of a
    window, the largest last rms residual among them).  A refinement that was asked to anchor (ba["anchor"], set by the drivers' refine_anchor) also says
    how many of its tracks were anchored -- the fewest and the most of a window -- since 0 means the solve ran free; one refined with Huber weights
    (ba["robust"]) how many of its measurements were down-weighted at the last iteration; otherwise the line is what it was."""
    def huber(measurements):
        if "robust" not in ba:
            return ""
        return f", huber {ba['robust']:g} px: {int(np.sum(ba['nout_last']))} of {int(measurements)} measurements down-weighted"

    if "window" in ba:
        anchors = f", {np.min(ba['nfix'])}-{np.max(ba['nfix'])} anchors" if "anchor" in ba else ""
        if "npart" in ba:  # refined with min_obs: how many of the windows' tracks live through part of their window, how many starts were triangulated
            anchors += f", {int(ba['npart'].sum())} partial of {int(ba['nt'].sum())}, {int(ba['ntri'].sum())} starts triangulated ({int(ba['nrej'].sum())} rejected)"
        anchors += huber(ba["nobs"].sum() if "nobs" in ba else ba["nt"].sum() * ba["window"])
        return (f"BA speed = {ba['speed_mean']:.2f} +/- {ba['speed_std']:.2f} km/h ({len(ba['first'])} windows of {ba['window']} frames, "
                f"{ba['nt'].min()}-{ba['nt'].max()} tracks{anchors}, f = {np.nanmax(ba['f_last']) if np.isfinite(ba['f_last']).any() else np.nan:.3f} pixels)")
    anchors = (f", {ba['nfix']} anchors" if "anchor" in ba else "") + (huber(ba["nt"] * len(ba["speed"])) if "robust" in ba else "")
    return f"BA speed = {ba['speed_mean']:.2f} +/- {ba['speed_std']:.2f} km/h ({ba['nt']:g} tracks{anchors}, f = {ba['f_last']:.3f} pixels)"


def _tag_anchor(ba, refine_anchor):
    """A clip's refinement (either form) marked with what it was asked to anchor; None: untouched."""
    return ba if refine_anchor is None or ba is None else dict(ba, anchor=refine_anchor)


def _check_robust(refine, refine_robust=None):
    """-> None (no Huber weights: the option is absent or 0), or the threshold in pixels; raises ValueError by name before anything is queued."""
    if refine_robust is None:
        return None
    if refine != "ba":
        raise ValueError("refine_robust needs refine='ba'")
    d = float(refine_robust)
    if not (np.isfinite(d) and d >= 0.0):
        raise ValueError(f"refine_robust = {refine_robust}: a finite number of pixels >= 0 (0 = off)")
    return d or None


def _check_refine(refine, refine_window=None, refine_stride=None, refine_anchor=None):
    """-> (refine is on, the window length or None, the stride or None); raises ValueError by name before anything is queued."""
    if refine not in (None, "ba"):
        raise ValueError(f"refine must be None or 'ba', got {refine!r}")
    if refine_anchor not in (None, "plate"):
        raise ValueError(f"refine_anchor must be None or 'plate', got {refine_anchor!r}")
    if refine_anchor is not None and refine != "ba":
        raise ValueError("refine_anchor needs refine='ba'")
    if refine_window is None:
        if refine_stride is not None:
            raise ValueError("refine_stride needs refine_window")
        return refine == "ba", None, None
    if refine != "ba":
        raise ValueError("refine_window needs refine='ba'")
    window = int(refine_window)
    if window < 2:
        raise ValueError(f"refine_window = {window}: a window needs at least two frames")
    if window > 256:
        raise ValueError(f"refine_window = {window}: at most 256 frames (the bundle adjustment's 255 free cameras)")
    stride = window - 1 if refine_stride is None else int(refine_stride)
    if not 1 <= stride <= window - 1:
        raise ValueError(f"refine_stride = {stride} is outside 1 .. refine_window - 1 = {window - 1}")
    return True, window, stride


def unpack_record(raw, lay):
    """A vh_session_record (uint8 array `raw`, offsets `lay`) as the dict TrackerSession.state() returns; every array is a copy."""
    n0, nh = lay.n0, lay.nhist

    def rd(off, count, dtype):
        return np.frombuffer(raw, dtype, count, off).copy()

    n_cur, n_pose, frame_i, klt_flags = (int(rd(off, 1, np.int32)[0]) for off in (lay.n_cur, lay.n_pose, lay.frame_i, lay.klt_flags))
    return dict(vg=rd(lay.vg, n0, np.uint8).astype(bool), vp=rd(lay.vp, n0, np.uint8).astype(bool), p=rd(lay.p, 2 * n_cur, np.float32).reshape(n_cur, 2),
                ids=rd(lay.ids, n_cur, np.int32), P=rd(lay.P, 5 * n0 * nh, np.float32).reshape(5, n0, nh), B=rd(lay.B, nh * 14, np.float32).reshape(nh, 14),
                S=rd(lay.S, nh * 9, np.float32).reshape(nh, 9), p3=rd(lay.p3, 3 * n0, np.float64).reshape(n0, 3), t=rd(lay.t, 3, np.float32),
                res=float(rd(lay.res, 1, np.float64)[0]), n_cur=n_cur, n_pose=n_pose, frame_i=frame_i, klt_flags=klt_flags,
                pose_info=rd(lay.pose_info, 2, np.int32))


class HostFrameFeeder:
    """Frame ingest from host memory: pinned staging buffers + a side HIP stream, double buffered,
    so the PCIe upload of frame i+1 overlaps the tracking of frame i.  `put(frames)` starts the upload of one frame per
    stream (numpy uint8 [H,W] arrays or a single [batch,H,W] array) and returns the slot; `get(slot)` makes the current
    stream wait for it and returns the device table of frame pointers for TrackerSession.step(frames_table=...);
    `after_step(slot)` hands the previous frame's buffer back.  depth >= 3 keeps the upload one frame ahead."""

    def __init__(self, batch, height, width, depth=3, lanes=None):
        torch = L.torch_cuda()
        self.torch, self.batch, self.depth = torch, batch, depth
        # one upload is split over `lanes` HIP streams (separate DMA engines).  Measured at 64 streams of 1080p (bench.py --host-frames, tools/exp/
        # host_feed_lanes.sh): 1 lane 21.7 k frames/s, 2 lanes 24.6 k (50.8 GB/s of the x16 Gen5 link), 4 lanes 24.1 k, 8 lanes 18.0 k
        import os

        self.lanes = max(1, min(batch, int(os.environ.get("VH_FEEDER_LANES", 0)) or (lanes or (2 if batch >= 8 else 1))))
        self.lane_streams = [torch.cuda.Stream() for _ in range(self.lanes - 1)]
        self.lane_done = [[torch.cuda.Event() for _ in range(self.lanes - 1)] for _ in range(depth)]
        self.pinned = [torch.empty((batch, height, width), dtype=torch.uint8).pin_memory() for _ in range(depth)]
        self.dev = [torch.empty((batch, height, width), dtype=torch.uint8, device="cuda") for _ in range(depth)]
        self.tables = [torch.tensor([self.dev[k][b].data_ptr() for b in range(batch)], dtype=torch.int64, device="cuda") for k in range(depth)]
        self.copy_stream = torch.cuda.Stream()
        self.ready = [torch.cuda.Event() for _ in range(depth)]
        self.free = [torch.cuda.Event() for _ in range(depth)]
        for e in self.free + self.ready:
            e.record()
        self.n = 0
        self._last = None

    def put(self, frames):
        """frames: a pinned torch uint8 tensor [batch,H,W] (uploaded in place, zero staging copies — the decoder should
        write there), or numpy arrays, which are first staged into this feeder's pinned slot."""
        torch = self.torch
        slot = self.n % self.depth
        self.n += 1
        if isinstance(frames, torch.Tensor) and frames.is_pinned():
            src = frames
        else:
            self.ready[slot].synchronize()  # the previous upload out of this staging slot must have finished
            src = self.pinned[slot]
            if isinstance(frames, np.ndarray) and frames.ndim == 3:
                src.numpy()[...] = frames
            else:
                for b, f in enumerate(frames):
                    src[b].numpy()[...] = f
        with torch.cuda.stream(self.copy_stream):
            self.copy_stream.wait_event(self.free[slot])  # the tracker is done with this device buffer
            if self.lanes == 1:
                self.dev[slot].copy_(src, non_blocking=True)
            else:
                bounds = [round(k * self.batch / self.lanes) for k in range(self.lanes + 1)]
                for k, st in enumerate(self.lane_streams):  # lanes 1.. on their own streams, lane 0 on the copy stream itself
                    a, b = bounds[k + 1], bounds[k + 2]
                    st.wait_event(self.free[slot])
                    with torch.cuda.stream(st):
                        self.dev[slot][a:b].copy_(src[a:b], non_blocking=True)
                        self.lane_done[slot][k].record(st)
                self.dev[slot][: bounds[1]].copy_(src[: bounds[1]], non_blocking=True)
                for ev in self.lane_done[slot]:
                    self.copy_stream.wait_event(ev)
            self.ready[slot].record(self.copy_stream)
        return slot

    def get(self, slot):
        self.torch.cuda.current_stream().wait_event(self.ready[slot])
        return self.tables[slot]

    def after_step(self, slot):
        """Call right after the step that consumed `slot` has been enqueued.  The frame of the PREVIOUS step was that step's
        im0 and is free from here on (a frame is read by two steps: as im1, then as im0)."""
        if self._last is not None:
            self.free[self._last].record(self.torch.cuda.current_stream())
        self._last = slot


# ----------------------------------------------------------------------------------------------------------------------------------
# the reference's driver (vidExample.py:52-178 minus decode and plots): frame-0 initialisation, the frame loop, the table and the summary
# ----------------------------------------------------------------------------------------------------------------------------------
TABLE_HEADER = ("\n" + "%13s" * 9) * 2 % ("image", "procTime", "pointTracks", "metric", "dt", "time", "dx", "distance", "speed",
                                         "#", "(s)", "#", "(pixels)", "(s)", "(s)", "(m)", "(m)", "(km/h)")  # vidExample.py:51-74
ROW_FORMAT = "{:13g}{:13.3f}{:13g}{:13.3f}{:13.3f}{:13.3f}{:13.2f}{:13.2f}{:13.1f}"  # vidExample.py:165


def table_row(S_row):
    """One line of the reference's results table (vidExample.py:164-165) from a 9-column float32 stats row."""
    return ROW_FORMAT.format(*tuple(S_row))


def summary_lines(S, n, frame_numbers, seconds):
    """The closing lines of the reference's run (vidExample.py:177-178)."""
    with np.errstate(all="ignore"):
        a = f"\nSpeed = {S[1:, 8].mean():.2f} +/- {S[1:, 8].std():.2f} km/h\nRes = {S[1:, 3].mean():.3f} pixels"
    b = f"Processed {n:g} images: {np.asarray(frame_numbers)[:]} in {seconds:.2f}s ({n / max(seconds, 1e-12):.2f}fps)\n"
    return [a, b]


@dataclasses.dataclass(frozen=True)
class Frame0Settings:
    """How frame 0 of a clip is initialised (vidExample.py:105-127): the plate, the ROI border around it, goodFeaturesToTrack's and cornerSubPix's
    arguments.  The defaults are the reference's call; the drivers build one from their keywords and hand it down whole."""
    plate: str = "Chile"
    roi_border: tuple = (700, 500)
    max_corners: int = 1000
    quality: float = 0.01
    block: int = 5
    harris_k: float = 0.04
    subpix: tuple = (5, 100, 0.001)
    use_harris: bool = True
    min_distance: float = 0.0

    def __post_init__(self):
        if not math.isfinite(float(self.min_distance)):
            raise ValueError(f"min_distance must be finite, got {self.min_distance}")

    @property
    def cap(self):
        """Track capacity of a session these settings fill: the 4 plate corners + max_corners."""
        return 4 + int(self.max_corners)

    @functools.cached_property
    def plate_w(self):
        """The plate's world points as the C ABI takes them: 12 contiguous float64."""
        from .common import worldPointsLicensePlate

        return np.ascontiguousarray(np.asarray(worldPointsLicensePlate(self.plate), np.float64).reshape(12))

    @property
    def reference_detector(self):
        """The reference's detector (vidExample.py:110: Harris, minDistance 0), which keeps the entry point it always used."""
        return bool(self.use_harris) and float(self.min_distance) == 0.0

    def outputs(self, nb):
        """Device outputs of a frame-0 batch call for nb clips: p, p3, vp, t, R, res, n."""
        torch, cap = L.torch_cuda(), self.cap
        layout = (((nb, cap, 2), torch.float32), ((nb, cap, 3), torch.float64), ((nb, cap), torch.uint8), ((nb, 3), torch.float32), ((nb, 9), torch.float64),
                  ((nb,), torch.float64), ((nb,), torch.int32))
        return tuple(torch.empty(shape, dtype=dtype, device="cuda") for shape, dtype in layout)


@dataclasses.dataclass(frozen=True)
class Replenish:
    """Replacing lost tracks with new corners (TrackerSession(replenish=...), vh_session_set_replenish; an extension beyond the reference, default off).
    every      a birth runs at a stream's own frame f when f > max(msv_frame, 0), (f - max(msv_frame, 0)) % every == 0 and f + baseline < nhist
    baseline   a newborn is triangulated from frames born .. born + baseline and joins the pose tracks at frame born + baseline if its point passes
    target     births refill a stream up to this many live tracks (None: the slot's frame-0 track count)
    max_new    corner budget of one birth (at most 2048)
    min_distance   new corners keep this distance (pixels) from each other and, as a square of that half-size, from every live track
    border     (x, y) pixels added around the bounding rectangle of the live tracks: the region searched
    max_reproj a newborn's point must reproject within this many pixels in every frame of its baseline (the reference's coarse forward-backward threshold)
    The detector and sub-pixel settings are the clip's Frame0Settings (quality, block, harris_k, use_harris, subpix)."""
    every: int = 5
    baseline: int = 5
    target: typing.Optional[int] = None
    max_new: int = 256
    min_distance: float = 10.0
    border: tuple = (0, 0)
    max_reproj: float = 1.0

    def __post_init__(self):
        if int(self.every) < 1 or int(self.baseline) < 1:
            raise ValueError(f"every and baseline must be at least 1, got {self.every}, {self.baseline}")
        if not 1 <= int(self.max_new) <= 2048:
            raise ValueError(f"max_new must be 1 .. 2048, got {self.max_new}")
        if self.target is not None and int(self.target) < 1:
            raise ValueError(f"target must be None or at least 1, got {self.target}")
        if not (math.isfinite(float(self.min_distance)) and math.isfinite(float(self.max_reproj))):
            raise ValueError("min_distance and max_reproj must be finite")


class Admitted(typing.NamedTuple):
    """What frame 0 of a clip leaves besides the stream's state: the ROIs (host ints) and the plate pose -- R0 [9] float64, res0 [1] float64: device
    views out of TrackerSession.admit, host values (R0 [3, 3], res0 a float) into clip_result."""
    boxa: tuple
    boxb: tuple
    R0: object
    res0: object

    def host(self):
        """The device views read back (waits for the stream)."""
        return self._replace(R0=self.R0.cpu().numpy(), res0=float(self.res0.item()))


def _to_device(frames, non_blocking=False):
    """uint8 gray frames (numpy arrays or torch tensors) -> dense CUDA tensors, uploaded on the current stream; CUDA tensors are used in place."""
    torch = L.torch_cuda()
    return [(f if isinstance(f, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(f))).cuda(non_blocking=non_blocking).contiguous() for f in frames]


def _frame0_batch_call(ws, frames0, qs, K64, settings, bufs):
    """vh_frame0_init_batch (the reference's detector) or vh_frame0_init_batch2 (any other) on the current stream: frames0 = dense CUDA [H, W] frames of
    one size, qs = their plate corners, bufs = settings.outputs(len(frames0)).  -> host list of nb x 8 ROIs (boxa, boxb)."""
    s, lib, nb = settings, ws.lib, len(frames0)
    H, W = frames0[0].shape
    q = np.ascontiguousarray(np.stack([np.asarray(x, np.float32).reshape(4, 2) for x in qs]))
    ptrs = (C.c_void_p * nb)(*[f.data_ptr() for f in frames0])
    rois = (C.c_int * (8 * nb))()
    win, it, eps = s.subpix
    if s.reference_detector:
        fn, name, detector = lib.vh_frame0_init_batch, "vh_frame0_init_batch", ()
    else:
        fn, name, detector = lib.vh_frame0_init_batch2, "vh_frame0_init_batch2", (1 if s.use_harris else 0, float(s.min_distance))
    L.check(fn(ws.handle, nb, C.cast(ptrs, C.c_void_p), W, H, W, q.ctypes.data_as(L.f32p), K64.ctypes.data_as(L.f64p), s.plate_w.ctypes.data_as(L.f64p),
               int(s.roi_border[0]), int(s.roi_border[1]), int(s.max_corners), float(s.quality), int(s.block), float(s.harris_k), *detector, int(win), int(it),
               float(eps), *[L.dptr(x) for x in bufs], rois, L.stream_ptr()), name)
    return list(rois)


def _frame0_batch3_call(ws, frames0, qs, Ks, settings, bufs):
    """vh_frame0_init_batch3 on the current stream: dense CUDA [H_b, W_b] frames of any sizes, their plate corners and their intrinsics (one K per clip).
    -> host list of nb x 8 ROIs (boxa, boxb)."""
    s, lib, nb = settings, ws.lib, len(frames0)
    q = np.ascontiguousarray(np.stack([np.asarray(x, np.float32).reshape(4, 2) for x in qs]))
    ptrs = (C.c_void_p * nb)(*[f.data_ptr() for f in frames0])
    cams = (L.ClipCamera * nb)(*[L.clip_camera(f.shape[1], f.shape[0], K) for f, K in zip(frames0, Ks)])
    rois = (C.c_int * (8 * nb))()
    win, it, eps = s.subpix
    L.check(lib.vh_frame0_init_batch3(ws.handle, nb, C.cast(ptrs, C.c_void_p), cams, q.ctypes.data_as(L.f32p), s.plate_w.ctypes.data_as(L.f64p),
                                      int(s.roi_border[0]), int(s.roi_border[1]), int(s.max_corners), float(s.quality), int(s.block), float(s.harris_k),
                                      1 if s.use_harris else 0, float(s.min_distance), int(win), int(it), float(eps), *[L.dptr(x) for x in bufs], rois,
                                      L.stream_ptr()), "vh_frame0_init_batch3")
    return list(rois)


def frame0_batch(frames, qs, K, plate="Chile", roi_border=(700, 500), max_corners=1000, quality=0.01, block=5, harris_k=0.04, subpix=(5, 100, 0.001),
                 use_harris=True, min_distance=0.0):
    """Frame 0 of many clips at once (vidExample.py:105-127 for each): `frames` = the clips' first frames (numpy / torch uint8 [H, W] of one size, or one
    [B, H, W] array), `qs` = their plate corners [4, 2].  One vh_frame0_init_batch launch sequence for all of them.  Returns one dict per clip with the keys
    of the oracle's frame0: p [n, 2] (the 4 plate corners, then the refined corners), p3 [n, 3], vp [n] bool, t [3], R [3, 3], res, boxa, boxb.
    use_harris=False: Shi-Tomasi (minimum eigenvalue) corners; min_distance >= 1: corners at least that far apart (vh_frame0_init_batch2)."""
    settings = Frame0Settings(plate, roi_border, max_corners, quality, block, harris_k, subpix, use_harris, min_distance)
    torch = L.torch_cuda()
    dev = _to_device(frames)
    H, W = dev[0].shape
    assert all(d.shape == (H, W) and d.dtype == torch.uint8 for d in dev), "frames must be uint8 and share one size"
    bufs = settings.outputs(len(dev))
    rois = _frame0_batch_call(L.workspace(W, H), dev, qs, L.host_K(K), settings, bufs)
    p, p3, vp, t0, R0, res0, n0 = (x.cpu().numpy() for x in bufs)
    out = []
    for b in range(len(dev)):
        k = int(n0[b])
        out.append(dict(p=p[b, :k].copy(), p3=p3[b, :k].copy(), vp=vp[b, :k].astype(bool), t=t0[b].copy(), R=R0[b].reshape(3, 3).copy(), res=float(res0[b]),
                        boxa=tuple(rois[8 * b:8 * b + 4]), boxb=tuple(rois[8 * b + 4:8 * b + 8])))
    return out


def replenish_result(st, n, baseline):
    """What the replenishment did in a clip of n frames, from the stream's state with born / tri / n_rows (a pure function): per-frame counts of the rows
    born, promoted (at born + baseline) and rejected there (alive at that frame, not triangulated), the rows left, and per row its birth frame and tri."""
    k = int(st["n_rows"])
    born, tri = np.asarray(st["born"][:k], np.int32), np.asarray(st["tri"][:k], np.uint8)
    new = born > 0
    due = np.minimum(born + int(baseline), n - 1)
    judged = new & (born + int(baseline) <= n - 1) & np.isfinite(st["P"][4, np.arange(k), due])

    def per_frame(rows):
        return np.bincount(born[rows] + int(baseline), minlength=n)[:n].astype(np.int64)

    return dict(born=np.bincount(born[new], minlength=n)[:n].astype(np.int64), promoted=per_frame(new & (tri == 1)), rejected=per_frame(judged & (tri == 0)),
                rows_left=int(len(st["vg"]) - k), born_frame=born.copy(), tri=tri.copy())


def replenish_line(r):
    return f"Replenish: {int(r['born'].sum())} tracks born, {int(r['promoted'].sum())} promoted, {int(r['rejected'].sum())} rejected, {r['rows_left']} rows left"


def clip_result(st, clip, f0, seconds, step_seconds, sessions, recoveries, proc=None, ba=None, replenish=None):
    """THE result of a clip, whichever driver ran it (a pure function: numpy in, fresh arrays out, no device).
    st       the stream's state after the clip's last frame (TrackerSession.state / ExportedState.result).  Its session may have been sized for longer
             clips and has room for 4 + max_corners tracks: the history is cut to the clip's n frames and to the k tracks frame 0 found (S[0, 2]:
             k_sess_init writes the count there; rows beyond them never existed)
    clip     dict(n, name, frame_numbers); f0: the clip's Admitted with host values
    seconds  the wall time the `Processed ...` line reports; step_seconds: the mean time of a frame step, which rows 1.. of the procTime column carry
             (row 0: 0) unless `proc` gives the column frame by frame (run_sequence's live table)
    ba       the clip's refinement (unpack_refine's dict; None: not asked for): the result gains the key "ba" and the lines gain ba_line(ba) at the end
    replenish  the clip's Replenish (None: the option was off): st then carries born / tri / n_rows, the track rows are cut to the n_rows the births
             used instead of to the k of frame 0, and the result gains "replenish" (replenish_result) and one line behind the summary
    `lines` = the start line, TABLE_HEADER, one table_row per frame and the two summary_lines."""
    n, k = clip["n"], int(st["S"][0, 2])
    k0 = k
    if replenish is not None:
        k = int(st["n_rows"])
    S = st["S"][:n].copy()
    S[0, 1] = 0.0
    S[1:, 1] = step_seconds
    if proc is not None:
        S[:, 1] = proc
    B = st["B"][:n].copy()
    lines = [f"Starting image processing on {clip['name']} ...", TABLE_HEADER] + [table_row(S[i]) for i in range(n)]  # vidExample.py:50
    lines += summary_lines(S, n, clip["frame_numbers"], seconds)
    extra = {}
    if replenish is not None:
        extra["replenish"] = replenish_result(st, n, replenish.baseline)
        lines.append(replenish_line(extra["replenish"]))
    if ba is not None:
        lines.append(ba_line(ba))
        extra["ba"] = ba
    return dict(S=S, B=B, P=st["P"][:, :k, :n].copy(), vg=st["vg"][:k].copy(), vp=st["vp"][:k].copy(), p=st["p"].copy(), p3=st["p3"][:k].copy(),
                ids=st["ids"].copy(), n_tracks0=k0, t0=B[0, 0:3].copy(), R0=np.array(f0.R0, np.float64).reshape(3, 3), res0=float(f0.res0), boxa=tuple(f0.boxa),
                boxb=tuple(f0.boxb), klt_flags=st["klt_flags"], recoveries=recoveries, lines=lines, seconds=seconds, ms_per_frame=1e3 * step_seconds,
                sessions=sessions, **extra)


def run_sequence(frames, q, K, fps=None, times=None, frame_numbers=None, plate="Chile", roi_border=(700, 500), max_corners=1000, quality=0.01,
                 block=5, harris_k=0.04, subpix=(5, 100, 0.001), msv_frame=5, lk_coarse=None, lk_fine=None, route="session", live=True,
                 out=print, clock=None, name="sequence", use_harris=True, min_distance=0.0, fallback=False, fallback_params=None, refine=None,
                 refine_window=None, refine_stride=None, refine_anchor=None, replenish=None, spare=0, refine_min_obs=None,
                 refine_start_reproj=None, refine_robust=None):
    """The packaged counterpart of vidExample.py:52-178 (minus video decode and plots) on one clip.

    frames  sequence of n uint8 [H, W] gray frames (numpy arrays or CUDA tensors): what `cv2.cvtColor(cap.read(), BGR2GRAY)` / `cv2.imread(.., 0)` hands
            the reference's loop (vidExample.py:89-93)
    q       float32 [4, 2]: the hand-clicked plate corners of frame 0 (the .mat file's `q`, vidExample.py:31-32)
    K       the camera's 3 x 3 intrinsic matrix, reference layout (images.py:148-151)
    fps / times / frame_numbers   B[i, 12] (seconds; `CAP_PROP_POS_MSEC / 1000` or the EXIF time) and B[i, 13] per frame: either `times` or `fps`
    route   "session": frame 0 as a batch of one clip (TrackerSession.admit: Harris -> cornerSubPix -> plate pose -> image2world -> insidebbox, ONE device sequence) straight
            into a device-resident TrackerSession -- nothing but the frames goes up and nothing but the printed rows comes down (the only route of the
            product; a host loop on the drop-in functions -- what INTEGRATION.md's import switch gives a maintainer -- lives in tools/dropin_loop.py as a
            measurement harness).
    live    True prints every row as its frame finishes (one small read-back per frame, like the reference); False runs the whole clip first.
    use_harris, min_distance   the frame-0 detector (goodFeaturesToTrack's useHarrisDetector / minDistance; the defaults are the reference's call; any
            other setting goes through vh_frame0_init_batch2).
    fallback   True: a frame whose coarse KLT stage fails recovers the motion by feature matching (TrackerSession(fallback=True): one host read per
            frame step; default off).  The result then carries `recoveries` = [the recovery ran, it found a model] counts.
    refine  None (default: nothing new is queued), or "ba": after the last frame the clip is bundle-adjusted on the device (TrackerSession.refine:
            vidExample.py:157's fcnNLS_batch over all frames and surviving tracks); the result gains "ba" and one line follows the summary (ba_line).
    refine_window, refine_stride   None (default): the whole clip, as above -- at most 256 frames.  refine_window=W (2 .. 256; needs refine="ba"): a clip of
            at least W frames, of ANY length, is refined in windows of W frames starting at refine_window_starts(n, W, refine_stride) (default stride
            W - 1), all in one TrackerSession.refine_windows request, each on the tracks alive through it; "ba" is then merge_window_speeds' dict
            (speed, cover, speed_mean, speed_std and the per-window first, nt, iterations, converged, f_last) plus `window` and `stride`.  A clip
            shorter than W is refined whole.  The windows are independent solves and the merged speed an average of their estimates, not one global
            adjustment; without refine_anchor each window's scale is still held only by the damping.
    refine_anchor   None (default), or "plate" (needs refine="ba"): the clip's tracks 0..3 -- the plate corners, whose frame-0 world coordinates come from
            the plate's known size -- are held fixed in the adjustment (TrackerSession.set_anchors right after frame 0), which pins its scale to the
            plate.  "ba" gains nothing but `anchor`; its `nfix` says how many anchors were alive (per window in the windowed form: 0 = that window ran
            free), and the BA line says so too.  What it does not do: a window with first > 0 places its anchors by the tracker's own B[first, 3:6],
            windows stay separate solves, and the plate's frame-0 pose error is inherited.
    refine_min_obs, refine_start_reproj   None (default: nothing changes), or M >= 2 (needs refine="ba"): a window also takes the tracks observed in at
            least M of its frames (cut to the window's length) that have a world point to start from -- and, with refine_start_reproj = R > 0 pixels,
            those whose two-view start reprojects within R (TrackerSession.refine_windows(min_obs=, start_reproj=)).  Without refine_window the clip is
            ONE window of its own length (at most 256 frames).  "ba" is then the windowed dict plus, per window, nobs, npart, ntri, nrej, and the BA
            line says how many tracks are partial and how many starts were triangulated.
    refine_robust   None (default: plain least squares, nothing changes), or the Huber threshold D in pixels (needs refine="ba"): in every iteration a
            measurement whose reprojection error |r| exceeds D is weighted by D / |r| (TrackerSession.set_refine_robust), so a few wrong measurements
            no longer decide the speed.  "ba" gains `robust`, `nout_first` and `nout_last` (per window in the windowed form): how many measurements
            were down-weighted at the first and the last iteration, and the BA line says the latter.  f stays the unweighted rms residual.  What it
            does not do: choose D, or any loss but Huber's.
    replenish, spare   None (default: nothing new is queued), or a Replenish: the session gets `spare` rows behind the 4 + max_corners of frame 0, lost
            tracks are replaced by new corners there and triangulated on the device (TrackerSession(replenish=...); detector and sub-pixel settings: the
            frame-0 ones).  The result's track rows are then the rows used, it gains "replenish" (replenish_result) and one line follows the summary.
    out     line sink (default print); clock: time source for the procTime column / fps line (default time.perf_counter).

    Prints the reference's header, one 9-column row per frame (vidExample.py:165) and the `Speed = ... +/- ... km/h / Res = ...` summary (:177-178).
    Returns clip_result's dict (sessions = 1)."""
    import time as _time

    settings = Frame0Settings(plate, roi_border, max_corners, quality, block, harris_k, subpix, use_harris, min_distance)
    partial = _check_partial(refine, refine_min_obs, refine_start_reproj)
    robust = _check_robust(refine, refine_robust)
    refine, win, stride = _check_refine(refine, refine_window, refine_stride, refine_anchor)
    if route != "session":
        raise ValueError("route must be 'session' (the host loop on the drop-in functions is a measurement harness: tools/dropin_loop.py::run_sequence_dropin)")
    clock = clock or _time.perf_counter
    emit = out or (lambda line: None)
    n = len(frames)
    assert n >= 2, "a clip needs at least two frames"
    if times is None:
        assert fps, "give `times` or `fps`"
        times = [k / fps for k in range(n)]
    times = [np.float32(t) for t in times]
    frame_numbers = list(range(n)) if frame_numbers is None else list(frame_numbers)
    emit(f"Starting image processing on {name} ...")  # vidExample.py:50
    emit(TABLE_HEADER)
    t_begin = tic = clock()
    dev = _to_device(frames, non_blocking=True)
    H, W = dev[0].shape
    ses = _SessionSet(1, 1, max_corners).create(K, W, H, settings, n, lk_coarse=lk_coarse, lk_fine=lk_fine, msv_frame=msv_frame, fallback=fallback,
                                                 fallback_params=fallback_params, refine_robust=robust, **_replenish_kw(replenish, spare, settings))[0]
    f0 = ses.admit([(0, dev[0], q, times[0], frame_numbers[0])], settings, anchor=refine_anchor)[0]
    view = ses.view(0)
    proc = np.zeros(n)

    def row(i):  # the live table: one 36-byte read-back (synchronises, like the reference's print)
        r = ses._rd(C.c_void_p(view.S + 4 * 9 * i), 9, np.float32)
        proc[i] = r[1] = clock() - tic
        emit(table_row(r))

    if live:
        row(0)
    t_loop = clock()
    for i in range(1, n):
        tic = clock()
        ses.step([dev[i]], time_s=float(times[i]), frame_no=float(frame_numbers[i]))
        if live:
            row(i)
    ses.torch.cuda.synchronize()
    step_seconds = (clock() - t_loop) / (n - 1)
    ba = None
    if refine:
        (rh, ba_of), = _refine_finished(ses, [(0, n, None)], win, stride, partial)
        ba = _tag_anchor(ba_of(rh.result()), refine_anchor)
    st, recoveries, f0 = ses.state(0), ses.recoveries()[0], f0.host()
    res = clip_result(st, dict(n=n, name=name, frame_numbers=frame_numbers), f0, clock() - t_begin, step_seconds, 1, recoveries, proc if live else None, ba,
                      replenish=replenish)
    tail = 2 + (1 if refine else 0) + (1 if replenish is not None else 0)
    for line in res["lines"][-tail if live else 2:]:  # (not live: the whole clip ran first, and every row carries the mean time per frame)
        emit(line)
    return res


def _replenish_kw(replenish, spare, settings):
    """The TrackerSession keywords of a driver's replenish / spare arguments (none when the option is off and no spare rows are asked for)."""
    if replenish is None and not spare:
        return {}
    return dict(replenish=replenish, spare=int(spare), replenish_settings=settings)


def session_groups(streams, tracks=2000):
    """How many TrackerSessions (each on its own HIP stream) to split `streams` resident video streams of ~`tracks` tracks each into.  The stages of a frame
    step that run ONE workgroup per stream (RANSAC, bookkeeping + pose, the glue kernels) leave the chip nearly idle; with a second session on another HIP
    stream they run while that session's LK launches fill it.  Measured on one MI355X, C2 streams (2000 tracks), frames/s with 1 / 2 / 4 sessions: 2 streams 8.4 /
    8.9 k, 4: 14.0 / 15.1 / 15.0 k, 8: 20.4 / 22.4 / 23.6 k, 16: 28.5 / 30.6 / 31.3 k, 32: 35.0 / 37.7 / 38.1 k, 64: 40.4 / 41.9 / 41.3 k, 128: - / 44.8 / 43.6 k,
    256: 44.5 / 45.7 / 45.7 k; 8 sessions lose everywhere (a session of one or two streams falls back to the one-track-per-wavefront kernels).  A session
    needs enough tracks for the batched kernels: 8 streams of the real stills (278 tracks) LOSE 13 % as four sessions (19.8 -> 17.2 k), so the count is halved
    until a session holds at least 2000 tracks."""
    if streams < 2:
        return 1
    g = 4 if (8 <= streams < 64 and streams % 4 == 0) else (2 if streams % 2 == 0 else 1)
    while g > 1 and (streams // g) * max(int(tracks), 1) < 2000:
        g //= 2
    return g


_SIDE_STREAMS = {}


def session_streams(n):
    """The HIP streams `n` concurrent sessions run on: torch's current stream + n - 1 side streams that are created ONCE per device and handed out again on
    every call.  The runtime multiplexes HIP streams onto a few hardware queues (4 by default, GPU_MAX_HW_QUEUES); a process that keeps creating streams ends
    up with two "concurrent" sessions on one queue -- measured: a two-session leg that ran after a dozen earlier streams had been created fell from 38.7 k to
    36.2 k frames/s, a four-session one from 16.4 k to 11.0 k -- so the side streams are a fixed, small set."""
    torch = L.torch_cuda()
    dev = torch.cuda.current_device()
    pool = _SIDE_STREAMS.setdefault(dev, [])
    while len(pool) < n - 1:
        pool.append(torch.cuda.Stream(device=dev))
    return [torch.cuda.current_stream()] + pool[: max(n - 1, 0)]


def _slot_split(streams, sessions):
    """Slots per session: `streams` slots in contiguous blocks over `sessions` sessions."""
    owner = [b * sessions // streams for b in range(streams)]
    return [owner.count(g) for g in range(sessions)]


class _SessionSet:
    """`streams` resident streams as TrackerSessions, each on its own HIP stream of the pool: `sessions` of them (0 = auto, session_groups(streams, tracks)),
    never more than streams.  sizes[g]: the slots of session g; first[g]: the index of its slot 0 among all the streams (contiguous blocks);
    hip_streams[g]: the stream everything of session g is issued on (a session's context serves one HIP stream)."""

    def __init__(self, streams, sessions, tracks):
        G = int(sessions) if sessions and sessions > 0 else session_groups(streams, tracks)
        self.sizes = _slot_split(streams, max(1, min(G, streams)))
        self.first = [sum(self.sizes[:g]) for g in range(len(self.sizes))]
        self.hip_streams = session_streams(len(self.sizes))
        self.sess = []

    def create(self, K, W, H, settings, nhist, **session_kw):
        """The sessions, once the frame size is known: W x H frames, room for settings.cap tracks and nhist frames per stream."""
        torch = L.torch_cuda()
        for hs, size in zip(self.hip_streams, self.sizes):
            with torch.cuda.stream(hs):
                self.sess.append(TrackerSession(K, W, H, settings.cap, nhist=nhist, batch=size, **session_kw))
        return self.sess


def run_sequences(clips, K, plate="Chile", roi_border=(700, 500), max_corners=1000, quality=0.01, block=5, harris_k=0.04, subpix=(5, 100, 0.001),
                  msv_frame=5, lk_coarse=None, lk_fine=None, out=None, sessions=0, use_harris=True, min_distance=0.0, fallback=False, fallback_params=None, refine=None,
                  refine_window=None, refine_stride=None, refine_anchor=None, replenish=None, spare=0, refine_min_obs=None,
                 refine_start_reproj=None, refine_robust=None):
    """Many clips at once: the throughput form of run_sequence.  `clips` = list of dict(frames, q, times[, frame_numbers, name, K]) of ONE length -- the
    frame size and the intrinsics are each clip's own ("K": that clip's camera, default the K argument); the sessions are created at the elementwise
    maximum of the sizes and a frame step is sized for it, so clips of one camera type batch best.  One length stays required: a step advances every
    stream, and clips of other lengths belong to run_queue.  Every clip is a stream of a device-resident TrackerSession, so a frame step is one launch sequence for all the clips of a session
    (vh_session_step_v: each stream has its own clock).  `sessions`: the clips are split into this many sessions, each on its own HIP stream (0 = auto,
    session_groups(len(clips)): their one-workgroup-per-stream stages overlap the others' LK launches); results do not depend on it.  Frame 0 of the clips
    of a session is ONE TrackerSession.admit (one frame-0 batch call on the device, its outputs feed vh_session_init_dev directly); nothing is read back
    before the last frame.  use_harris / min_distance: the frame-0 detector, as in run_sequence.  fallback: the recovery by feature matching, as in
    run_sequence (the failed streams of a session share one vh_match_affine_batch call per step).  Returns one result dict per clip (clip_result's;
    `lines` = that clip's table and summary, printed through `out` if given), each equal to what run_sequence returns for the clip alone.  refine="ba": as in
    run_sequence; all the clips of a session are refined by ONE TrackerSession.refine after the last frame -- with refine_window=W (and clips of at least
    W frames) all the windows of all the clips of a session by ONE TrackerSession.refine_windows request.  refine_anchor="plate": as in run_sequence,
    for every clip.  refine_min_obs, refine_start_reproj: as in run_sequence (without refine_window: the clips of a session are ONE request of
    one-window clips).  refine_robust: as in run_sequence, for every clip.  replenish, spare: as in run_sequence, for every clip (the births of all the
    streams of a session are one launch sequence)."""
    import time as _time

    partial = _check_partial(refine, refine_min_obs, refine_start_reproj)
    robust = _check_robust(refine, refine_robust)
    refine, win, stride = _check_refine(refine, refine_window, refine_stride, refine_anchor)
    settings = Frame0Settings(plate, roi_border, max_corners, quality, block, harris_k, subpix, use_harris, min_distance)
    torch = L.torch_cuda()
    nclip = len(clips)
    assert nclip >= 1
    n = len(clips[0]["frames"])
    dev = [_to_device(c["frames"]) for c in clips]
    assert all(len(d) == n for d in dev), "clips must share one length (run_queue takes clips of any length)"
    assert all(f.shape == d[0].shape for d in dev for f in d), "the frames of a clip must share one size"
    H, W = max(d[0].shape[0] for d in dev), max(d[0].shape[1] for d in dev)
    group = _SessionSet(nclip, sessions, max_corners)
    for hs in group.hip_streams[1:]:
        hs.wait_stream(group.hip_streams[0])  # the frame uploads above ran on the current stream
    sess = group.create(K, W, H, settings, n, lk_coarse=lk_coarse, lk_fine=lk_fine, msv_frame=msv_frame, fallback=fallback, fallback_params=fallback_params,
                        refine_robust=robust, **_replenish_kw(replenish, spare, settings))
    members = [list(range(a, a + size)) for a, size in zip(group.first, group.sizes)]  # session -> its clips, in slot order
    times = np.stack([np.asarray(c["times"], np.float32) for c in clips])  # [clip, frame]
    fnos = np.stack([np.asarray(c.get("frame_numbers", np.arange(n)), np.float32) for c in clips])
    t_begin = _time.perf_counter()
    f0, f0_events = [], []
    for ses, hs, mem in zip(sess, group.hip_streams, members):
        with torch.cuda.stream(hs):
            f0_events.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
            f0_events[-1][0].record()
            f0 += ses.admit([(j, dev[b][0], clips[b]["q"], times[b, 0], fnos[b, 0], clips[b].get("K")) for j, b in enumerate(mem)], settings, anchor=refine_anchor)
            f0_events[-1][1].record()
    t_loop = _time.perf_counter()
    for i in range(1, n):
        for ses, hs, mem in zip(sess, group.hip_streams, members):
            with torch.cuda.stream(hs):
                ses.step([dev[b][i] for b in mem], time_s=times[mem, i], frame_no=fnos[mem, i])
    torch.cuda.synchronize()
    step_seconds = (_time.perf_counter() - t_loop) / (n - 1)  # every row carries the mean time of a frame step (of ALL clips)
    refined = []
    if refine:
        for ses, hs, mem in zip(sess, group.hip_streams, members):
            with torch.cuda.stream(hs):  # (one length: ONE request per session)
                refined.append(_refine_finished(ses, [(j, n, None) for j in range(len(mem))], win, stride, partial))
        refined = [[ba_of(rh.result()) for rh, ba_of in per] for per in refined]
    seconds = _time.perf_counter() - t_begin
    # what tools/exp/queue_timing.py reads: device time of the frame-0 block of every session (events on its stream), to set beside run_queue's
    run_sequences.last_stats = dict(sessions=len(sess), steps=n - 1, admission_ms=float(sum(a.elapsed_time(b) for a, b in f0_events)), admissions=len(sess))
    results = []
    for g, (ses, mem) in enumerate(zip(sess, members)):
        for j, b in enumerate(mem):
            meta = dict(n=n, name=clips[b].get("name", f"clip {b}"), frame_numbers=clips[b].get("frame_numbers", list(range(n))))
            results.append(clip_result(ses.state(j), meta, f0[b].host(), seconds, step_seconds, len(sess), ses.recoveries()[j],
                                       ba=_tag_anchor(refined[g][j], refine_anchor) if refine else None, replenish=replenish))
            if out is not None:
                for ln in results[-1]["lines"]:
                    out(ln)
    return results


# ----------------------------------------------------------------------------------------------------------------------------------
# a queue of clips of any length on a fixed set of resident streams
# ----------------------------------------------------------------------------------------------------------------------------------
def _queue_steps(next_length, sizes):
    """The schedule of run_queue, one global step at a time.  `next_length()` hands out the length (frames, >= 2) of the next clip of the FIFO, or None when
    the queue is empty; it is called only when a slot is free, in (session, slot) order.  Yields per step dict(admit, frames, done):
      admit   [(session, slot, clip)]: the clips that take a free slot at this step -- their frame 0 is initialised before the sessions step;
      frames  [session][slot] -> (clip, frame index) the slot tracks in this step's launch sequence, or None: the slot is empty and sits the step out;
      done    [(session, slot, clip)]: the clips whose last frame this was -- exported and freed, so the slot is refilled at the very next step."""
    slots = [[None] * n for n in sizes]
    clip, empty = 0, False
    while True:
        admit = []
        for g, ses in enumerate(slots):
            for j, cur in enumerate(ses):
                if cur is None and not empty:
                    n = next_length()
                    if n is None:
                        empty = True
                        continue
                    if n < 2:
                        raise ValueError(f"clip {clip} has {n} frames: a clip needs at least two")
                    ses[j] = [clip, 1, int(n)]
                    admit.append((g, j, clip))
                    clip += 1
        if not any(cur is not None for ses in slots for cur in ses):
            return
        frames = [[None if cur is None else (cur[0], cur[1]) for cur in ses] for ses in slots]
        done = []
        for g, ses in enumerate(slots):
            for j, cur in enumerate(ses):
                if cur is not None:
                    cur[1] += 1
                    if cur[1] == cur[2]:
                        done.append((g, j, cur[0]))
                        ses[j] = None
        yield dict(admit=admit, frames=frames, done=done)


def queue_clip_fits(index, shape, max_size):
    """run_queue's size rule (a pure function: no device): clip `index` with frames of `shape` = (H, W) fits sessions created for max_size = (H, W) iff
    each side does -- a portrait frame does not fit a landscape session of the same area.  Raises the ValueError run_queue raises, else returns shape."""
    h, w = int(shape[0]), int(shape[1])
    mh, mw = int(max_size[0]), int(max_size[1])
    if h > mh or w > mw:
        raise ValueError(f"run_queue: clip {index} has {w} x {h} frames, larger than max_size = {mw} x {mh} (W x H)")
    return h, w


def queue_plan(lengths, streams, sessions=1):
    """The whole schedule run_queue follows for clips of these lengths (a pure function: no device): the list of the steps of _queue_steps.  Greedy and
    FIFO: at every global step each free slot takes the next waiting clip, in (session, slot) order; a clip of n frames is admitted (frame 0) and tracked
    (frame 1) in its first step and holds its slot for n - 1 consecutive steps."""
    it = iter(lengths)
    sessions = max(1, min(int(sessions), int(streams)))
    return list(_queue_steps(lambda: next(it, None), _slot_split(int(streams), sessions)))


def run_queue(clips, K, streams, max_frames=None, sessions=0, on_result=None, max_size=None, plate="Chile", roi_border=(700, 500), max_corners=1000, quality=0.01, block=5,
              harris_k=0.04, subpix=(5, 100, 0.001), msv_frame=5, lk_coarse=None, lk_fine=None, out=None, use_harris=True, min_distance=0.0, fallback=False,
              fallback_params=None, refine=None, refine_window=None, refine_stride=None, refine_anchor=None, replenish=None, spare=0, refine_min_obs=None,
                 refine_start_reproj=None, refine_robust=None):
    """A queue of clips of ANY length on `streams` resident streams: what run_sequences is for clips of one length.  `clips` = any iterable of
    dict(frames, q, times[, frame_numbers, name, K]), each of >= 2 frames and with its own frame size and intrinsics ("K": default the K argument); it is consumed lazily -- a clip is pulled when a slot is free
    for it and its frames go up then, so at most `streams` clips are resident -- and may hold more clips than fit on the device at once.
    max_frames   the sessions' history length: no clip may be longer (ValueError when it is admitted); required unless `clips` is a list.
    max_size     (H, W) of the largest frame a clip may have: the size the sessions (and the frame-0 scratch) are created for.  Without it they take the
                 size of the first clip pulled.  A later clip that does not fit (queue_clip_fits) raises ValueError naming the clip and both sizes --
                 before any of its frames goes up or anything is queued for it; the clips already resident run to their end and are delivered first.
    sessions     the slots are split over this many TrackerSessions, each on its own HIP stream (0 = auto, session_groups(streams)); results do not
                 depend on it.
    The schedule is queue_plan's: one shared FIFO; at every global step each free slot takes the next clip, all admissions of a session are ONE
    TrackerSession.admit (one frame-0 batch call + one vh_session_init_dev per slot) on the session's stream, then every session issues ONE step in which
    its empty slots sit out (vh_session_step_some); a clip that has just had its last frame is exported (TrackerSession.export: one launch, one copy) and
    its slot is free.
    With fallback=False the loop never waits for the device except for a result whose pinned buffer is needed again (a ring of 2 x streams) and at
    the end of the run; frames given as CUDA tensors are used in place, host frames are uploaded on a side stream.
    on_result(index, result) is called as results land (polled at every step, never waited for); returns the results in input order.  A result is
    clip_result's: P / B / S cut to the clip's own length and the track rows to n_tracks0; `lines` = the clip's table and summary.
    refine="ba": as in run_sequence.  The clips of a session that finish at the same step are refined on the session's stream right behind their
    exports, one TrackerSession.refine per clip length among them; the records travel with the exports and the slots are free at the next step as ever.
    refine_window=W (refine_stride: as in run_sequence): the clips of at least W frames that finish at a step go through ONE TrackerSession.refine_windows
    request of their session, whatever their lengths (their "ba" is the merged dict); the per-length calls remain for clips shorter than W.
    refine_anchor="plate": as in run_sequence, for every clip (a slot's anchors are set at its clip's admission and cleared by the next one).
    refine_robust=D: as in run_sequence, for every clip (a setting of the sessions, made when they are created).
    replenish, spare: as in run_sequence, for every clip.  A finished clip's born / tri are read right behind its export (vh_session_replenish_state
    waits for the device: with the option on the loop waits once per finished clip)."""
    import time as _time

    partial = _check_partial(refine, refine_min_obs, refine_start_reproj)
    robust = _check_robust(refine, refine_robust)
    refine, win, stride = _check_refine(refine, refine_window, refine_stride, refine_anchor)
    settings = Frame0Settings(plate, roi_border, max_corners, quality, block, harris_k, subpix, use_harris, min_distance)
    torch = L.torch_cuda()
    if max_frames is None:
        if not isinstance(clips, (list, tuple)):
            raise ValueError("run_queue: max_frames is required unless `clips` is a list")
        max_frames = max(len(c["frames"]) for c in clips)
    nhist, streams = int(max_frames), int(streams)
    assert streams >= 1 and nhist >= 2
    group = _SessionSet(streams, sessions, max_corners)
    G, sess = len(group.sizes), group.sess
    main, upload = group.hip_streams[0], _upload_stream()
    source = iter(clips)
    pulled = {}          # clip index -> the clip as its slot uses it (dropped when the clip is done)
    size = [None if max_size is None else (int(max_size[0]), int(max_size[1]))]  # (H, W) the sessions are created for
    misfit = []          # the ValueError of a clip that does not fit: the queue ends there, the resident clips are finished and delivered, then it is raised

    def next_length():
        c = next(source, None)
        if c is None:
            return None
        k = next_length.count
        n = len(c["frames"])
        if n > nhist:
            raise ValueError(f"run_queue: clip {k} has {n} frames, more than max_frames = {nhist}")
        if n >= 2:
            shape = tuple(c["frames"][0].shape)
            size[0] = size[0] or shape
            try:
                queue_clip_fits(k, shape, size[0])
            except ValueError as e:
                misfit.append(e)
                return None
            host = [f for f in c["frames"] if not (isinstance(f, torch.Tensor) and f.is_cuda)]
            with torch.cuda.stream(upload if host else main):  # (host frames: an upload that waits for nothing the sessions have queued)
                dev = _to_device(c["frames"], non_blocking=True)
            assert all(d.shape == shape and d.dtype == torch.uint8 for d in dev), "the frames of a clip must share one size"
            pulled[k] = dict(dev=dev, uploaded=bool(host), q=c["q"], K=c.get("K"), times=np.asarray(c["times"], np.float32),
                             fnos=np.asarray(c.get("frame_numbers", np.arange(n)), np.float32), frame_numbers=c.get("frame_numbers", list(range(n))),
                             name=c.get("name", f"clip {k}"), n=n)
        next_length.count += 1
        return n

    next_length.count = 0
    ring, ring_i = [], 0   # pinned records + frame-0 extras, 2 x streams of them; entry: [record, extras, the job whose result it holds or None]
    pending, results, t_admit = [], {}, []   # pending: the ring entries that hold a job, oldest first
    t_begin = _time.perf_counter()

    def deliver(entry):
        handle, index, clip, f0, t0, ba = entry[2][:6]
        st = handle.result()
        if replenish is not None:
            st.update(entry[2][6])
        if ba is not None:
            ba = _tag_anchor(ba[1](ba[0].result()), refine_anchor)
        x = entry[1].numpy().copy()
        seconds = _time.perf_counter() - t0  # the clip's time in the queue: every row carries the mean over its frame steps
        res = results[index] = clip_result(st, clip, f0._replace(R0=x[0:9], res0=x[9]), seconds, seconds / (clip["n"] - 1), G, handle.recoveries, ba=ba, replenish=replenish)
        entry[2] = None
        pending[:] = [e for e in pending if e is not entry]
        if out is not None:
            for ln in res["lines"]:
                out(ln)
        if on_result is not None:
            on_result(index, res)

    def poll():
        for entry in [e for e in pending if e[2][0].done() and (e[2][5] is None or e[2][5][0].done())]:
            deliver(entry)

    held = [[None] * n for n in group.sizes]  # per slot: (the resident clip's Admitted, its admission time)
    idle_slots = steps = 0
    for step in _queue_steps(next_length, group.sizes):
        poll()
        if not sess:  # the first clips have been pulled: the (largest) frame size is known
            H, W = size[0]
            group.create(K, W, H, settings, nhist, lk_coarse=lk_coarse, lk_fine=lk_fine, msv_frame=msv_frame, fallback=fallback, fallback_params=fallback_params,
                         refine_robust=robust, **_replenish_kw(replenish, spare, settings))
            for ses, hs in zip(sess, group.hip_streams):
                with torch.cuda.stream(hs):  # the frame-0 scratch for a full house, so that no later admission grows it (growing waits for the stream)
                    L.check(ses.lib.vh_init_reserve_batch(ses.ws.handle, ses.batch, W, H, L.stream_ptr()), "vh_init_reserve_batch")
            rec_bytes = sess[0].record_layout().bytes
            ba_bytes = sess[0].refine_layout().bytes if refine else 0
            if win and nhist >= win:  # room for the most windows a clip of nhist frames can have (a clip shorter than W: the whole-clip record)
                win_bytes = sess[0].refine_window_layout(win, partial=partial is not None).bytes
                ba_bytes = max(ba_bytes, len(refine_window_starts(nhist, win, stride)) * win_bytes)
            if partial is not None:  # a clip that is not windowed: one window of its own length
                ba_bytes = max(ba_bytes, sess[0].refine_window_layout(min(nhist, 256), partial=True).bytes)
            ring = [[torch.empty(rec_bytes, dtype=torch.uint8).pin_memory(), torch.empty(10, dtype=torch.float64).pin_memory(), None,
                     torch.empty(ba_bytes, dtype=torch.uint8).pin_memory() if refine else None] for _ in range(2 * streams)]
        for g, (ses, hs) in enumerate(zip(sess, group.hip_streams)):
            adm = [(j, pulled[k]) for gg, j, k in step["admit"] if gg == g]
            with torch.cuda.stream(hs):
                if adm:
                    if hs != main:
                        hs.wait_stream(main)   # frames the caller produced on the current stream
                    if any(c["uploaded"] for _, c in adm):
                        hs.wait_stream(upload)
                    for _, c in adm:
                        if c["uploaded"] or hs != main:  # frames allocated on another stream than the one that reads them
                            for f in c["dev"]:
                                f.record_stream(hs)
                    ev0 = torch.cuda.Event(enable_timing=True)
                    ev1 = torch.cuda.Event(enable_timing=True)
                    ev0.record()
                    f0s = ses.admit([(j, c["dev"][0], c["q"], c["times"][0], c["fnos"][0], c["K"]) for j, c in adm], settings, anchor=refine_anchor)
                    for (j, _), f0 in zip(adm, f0s):
                        held[g][j] = (f0, _time.perf_counter())
                    ev1.record()
                    t_admit.append((ev0, ev1))
                # ONE step of the session: a pointer per slot (null: the slot sits the step out), its clock, and the host's copy of who is active
                row = step["frames"][g]
                idle_slots += sum(e is None for e in row)
                if not any(row):
                    continue  # (nothing resident in this session: no launch sequence at all)
                ptrs = np.array([0 if e is None else pulled[e[0]]["dev"][e[1]].data_ptr() for e in row], np.int64)
                clk = np.array([[0.0 if e is None else pulled[e[0]]["times"][e[1]] for e in row], [0.0 if e is None else pulled[e[0]]["fnos"][e[1]] for e in row]],
                               np.float32)
                tab = torch.from_numpy(ptrs).pin_memory().cuda(non_blocking=True)  # (pinned staging: a pageable upload would wait for the stream)
                clk = torch.from_numpy(clk).pin_memory().cuda(non_blocking=True)
                ses._queue_keep = (tab, clk)
                ses.step(frames_table=tab, time_s=clk[0], frame_no=clk[1], active=(ptrs != 0).astype(np.uint8))
                finished = []  # (slot, clip length, ring entry) of the clips of this session that end here
                for gg, j, k in step["done"]:
                    if gg != g:
                        continue
                    entry = ring[ring_i % len(ring)]
                    ring_i += 1
                    if entry[2] is not None:
                        deliver(entry)  # the one wait of the loop: this pinned buffer still holds a result nobody has taken
                    f0, t0 = held[g][j]
                    handle = ses.export(j, out=entry[0])
                    # (the plate pose of frame 0 is no part of the stream's state: 80 bytes beside the record)
                    entry[1].copy_(torch.cat([f0.R0, f0.res0]), non_blocking=True)
                    handle.event.record()
                    c = pulled.pop(k)
                    extra = None
                    if replenish is not None:
                        born, tri, counts = ses.replenish_state(j)
                        extra = dict(born=born, tri=tri, n_rows=int(counts[0]))
                    entry[2] = [handle, k, dict(n=c["n"], name=c["name"], frame_numbers=c["frame_numbers"]), f0, t0, None, extra]
                    pending.append(entry)
                    held[g][j] = None
                    finished.append((j, c["n"], entry))
                if refine and finished:  # right behind the exports; a clip's records land in its own pinned buffer
                    for (_, _, e), ba in zip(finished, _refine_finished(ses, [(j, n, e[3]) for j, n, e in finished], win, stride, partial)):
                        e[2][5] = ba
        steps += 1
        poll()
    for hs in group.hip_streams:
        hs.synchronize()
    for entry in list(pending):
        deliver(entry)
    seconds = _time.perf_counter() - t_begin
    run_queue.last_stats = dict(steps=steps, sessions=G, mean_idle_slots=idle_slots / max(steps, 1), seconds=seconds,
                                admission_ms=float(sum(a.elapsed_time(b) for a, b in t_admit)), admissions=len(t_admit))
    if misfit:
        raise misfit[0]
    return [results[k] for k in range(next_length.count)]


_UPLOAD_STREAMS = {}


def _upload_stream():
    """The side stream run_queue uploads host frames on (one per device, created once, like the session streams)."""
    torch = L.torch_cuda()
    dev = torch.cuda.current_device()
    if dev not in _UPLOAD_STREAMS:
        _UPLOAD_STREAMS[dev] = torch.cuda.Stream(device=dev)
    return _UPLOAD_STREAMS[dev]


def main(argv=None):
    """`python -m velocity_amd.driver clip.npz [--seq b]`: the reference's run (`python vidExample.py`) on a decoded clip.
    clip.npz holds `<seq>_frames` uint8 [n, H, W], `<seq>_times` [n] seconds, `<seq>_q` [4, 2] plate corners and `<seq>_K` [3, 3] (the format of
    tests/golden/stills_gray.npz); decoding videos is out of scope (no decoder in the image)."""
    import argparse

    ap = argparse.ArgumentParser(description=main.__doc__)
    ap.add_argument("clip")
    ap.add_argument("--seq", default="b")
    ap.add_argument("--border", type=int, nargs=2, default=None, help="ROI border around the plate (vidExample.py:108 uses 700 500; the 1024 x 768 stills fixture needs 180 140)")
    ap.add_argument("--msv-frame", type=int, default=5)
    ap.add_argument("--min-distance", type=float, default=0.0, help="minimum distance between the frame-0 corners (vidExample.py:110 uses 0)")
    ap.add_argument("--fallback", action="store_true", help="recover the motion by feature matching when the coarse KLT stage fails (one host read per frame)")
    ap.add_argument("--refine", choices=["ba"], default=None, help="bundle-adjust the finished clip on the device and print the refined speed (vidExample.py:157)")
    ap.add_argument("--refine-window", type=int, default=None, metavar="W", help="with --refine ba: refine the clip in windows of W frames (2 .. 256); clips of any length")
    ap.add_argument("--refine-stride", type=int, default=None, metavar="S", help="frames between the starts of consecutive windows (1 .. W-1; default W-1)")
    ap.add_argument("--refine-min-obs", type=int, default=None, metavar="M",
                    help="with --refine ba: a window also takes the tracks observed in at least M of its frames (a clip without --refine-window: one window)")
    ap.add_argument("--refine-start-reproj", type=float, default=None, metavar="R",
                    help="with --refine-min-obs: tracks without a trusted world point start from a two-view triangulation that reprojects within R pixels")
    ap.add_argument("--refine-anchor", choices=["plate"], default=None, help="with --refine ba: hold the four plate corners fixed in the adjustment (a metric scale from the plate)")
    ap.add_argument("--refine-robust", type=float, default=None, metavar="PX",
                    help="with --refine ba: Huber weights, a measurement whose reprojection error exceeds PX pixels is down-weighted in every iteration")
    ap.add_argument("--replenish", type=int, nargs="?", const=5, default=None, metavar="EVERY",
                    help="replace lost tracks with new corners every EVERY frames (default 5) and triangulate them on the device")
    ap.add_argument("--spare", type=int, default=256, metavar="ROWS", help="with --replenish: rows for new tracks behind the frame-0 ones")
    ap.add_argument("--shi-tomasi", action="store_true", help="frame-0 corners by the minimum-eigenvalue detector instead of Harris")
    a = ap.parse_args(argv)
    d = np.load(a.clip)
    fr = d[f"{a.seq}_frames"]
    border = tuple(a.border) if a.border else ((700, 500) if fr.shape[2] >= 1900 else (180, 140))
    run_sequence(fr, d[f"{a.seq}_q"], d[f"{a.seq}_K"], times=d[f"{a.seq}_times"], roi_border=border, msv_frame=a.msv_frame,
                 name=f"{a.clip}:{a.seq}", use_harris=not a.shi_tomasi, min_distance=a.min_distance, fallback=a.fallback, refine=a.refine,
                 refine_window=a.refine_window, refine_stride=a.refine_stride, refine_anchor=a.refine_anchor,
                 refine_min_obs=a.refine_min_obs, refine_start_reproj=a.refine_start_reproj, refine_robust=a.refine_robust,
                 replenish=None if a.replenish is None else Replenish(every=a.replenish), spare=a.spare if a.replenish is not None else 0)


if __name__ == "__main__":
    main()
