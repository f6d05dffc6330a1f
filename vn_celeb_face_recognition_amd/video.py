"""Frame-stream control flow of demo_video.py / celeb_statistic.py (/root/reference/demo_video.py:46-199), the same
on one GPU and on N:

  * frames are cut into batches of --n_frames; batch b belongs to rank b % world (frames are independent units,
    demo_video.py:186-188).  A rank only READS its own batches (random-access sources skip the others' decode);
  * every rank uploads its batches through a pinned staging ring on a copy stream (upload.FrameUploader) and pushes
    them through `FacePipeline.submit` (detection stream + embedding stream, faces of consecutive batches embedded
    together); batches are retired two late, so the GPU always has work queued;
  * retiring round r (batches r*world .. r*world + world-1) is the ONE exchange step of the path: ONE
    fixed-size all-gather of each rank's (1 + cap, 512 + 4 + 1) fp32 block -- a header row with the face count, then
    embedding, box, frame slot per face (with `emotions=k` also the face's k emotion indices and probabilities: 2k more
    values per row) -- issued on a side stream behind the batch's own event.  Its result is read
    on the host one round LATER (pinned D2H + event), so no rank ever blocks on a collective it has just issued; a
    batch with more than `cap` faces is completed by one exactly-sized follow-up gather that every rank derives from
    the same header rows;
  * every rank issues the same collectives in the same order: rounds 0 .. ceil(batches / world) - 1, each exactly once
    (a rank without a batch in the last round sends an empty block), and nothing else in between;
  * rank 0 classifies the gathered embeddings (one vnf_classify per round) and collates tracker rows in frame order.
"""
import contextlib
from dataclasses import dataclass

import numpy as np
import torch
import torch.distributed as dist

from .pipeline import identify_names


def tracker_row(time_in_video, frame_idx, names, bboxes, frame_shape):
    """demo_video.py:155-168 (one CSV row)."""
    row = [str(time_in_video), '"' + str(names) + '"', str(frame_idx)]
    if len(bboxes) == 0:
        scaled_bboxes = []
    else:
        h, w, _ = frame_shape
        scale = np.array([w, h, w, h])
        # plain python floats: NumPy >= 2 would print np.float64(...) into the CSV, the reference's files hold bare numbers
        scaled_bboxes = [[float(v) for v in x / scale] for x in bboxes]
    row.append('"' + str(scaled_bboxes) + '"')
    return ','.join(row) + '\n'


class FrameSource:
    """Batches of a frame stream for one rank.  `frames` is either a random-access sequence (len + __getitem__: a list
    of image paths is decoded with `load`, an array is indexed) or a plain iterator (a decoder: the other ranks' frames
    are pulled and dropped).  Frame numbers start at 1 and time = number / fps, as demo_video.py:84-90 counts them.
    compressed: optional callable i -> the JPEG bytes of frame i of a random-access source, or None for a frame that is
    no JPEG (a Motion-JPEG AVI's chunks, the .jpg files of a directory): what `rank_batches(compressed=True)` yields.
    keep: optional predicate on the 1-based frame number (celeb_statistic.py:180-187, -fidx).  The source then yields
    only the frames it keeps, cut into batches by their position among the kept ones; number and time stay those of
    the original stream.  A random-access source never reads, let alone decodes, a frame it does not keep."""

    def __init__(self, frames, fps, load=None, compressed=None, keep=None):
        self.frames, self.fps, self.load = frames, float(fps), load
        self.compressed = compressed if (compressed is not None and hasattr(frames, "__getitem__")) else None
        self.random_access = hasattr(frames, "__getitem__") and hasattr(frames, "__len__")
        self.reads = 0   # frames this rank actually fetched (tests)
        self.total = len(frames) if self.random_access else None   # frames the source yields (iterators: known once exhausted)
        self.keep = self._kept = None
        if keep is not None:
            self.sample(keep)

    def sample(self, keep):
        """yield only the frames whose 1-based number `keep` accepts (before the first batch is drawn) -> self"""
        self.keep = keep
        if self.random_access:
            self._kept = [i for i in range(len(self.frames)) if keep(i + 1)]
            self.total = len(self._kept)
        else:
            self._kept = []                      # filled as the stream is pulled: every rank pulls every frame
        return self

    def number_of(self, pos):
        """the 1-based number, in the original stream, of the pos-th (0-based) frame this source yields.  A sequential
        source learns the numbers as it is pulled, so this is defined for the frames pulled so far only.  run_stream
        asks for the frames of a round it consumes, and a rank consumes round r only after it has drawn its own batch
        of round r + 1 (or exhausted the stream): every batch of round r has then passed through `rank_batches`."""
        return pos + 1 if self.keep is None else self._kept[pos] + 1

    def _get(self, i):
        self.reads += 1
        f = self.frames[i]
        return self.load(f) if self.load is not None else np.asarray(f)

    def _get_compressed(self, idx):
        """jpeg.CompressedBatch of the frames idx when every one of them is a JPEG, else None"""
        from .jpeg import CompressedBatch
        out = CompressedBatch()
        for i in idx:
            d = self.compressed(i)
            if d is None:
                return None
            out.append(d)
        self.reads += len(out)
        return out

    def rank_batches(self, n_frames, rank=0, world=1, compressed=False):
        """yields (batch_index, [frames], [[time, frame_number], ...]) for batches with batch_index % world == rank.
        compressed=True: a batch whose frames are all JPEGs comes as a jpeg.CompressedBatch of their bytes, not
        decoded; every other batch as decoded frames, as without it."""
        if self.random_access:
            total = self.total
            for b in range(rank, (total + n_frames - 1) // n_frames, world):
                idx = range(b * n_frames, min(total, (b + 1) * n_frames))
                if self._kept is not None:
                    idx = self._kept[idx.start:idx.stop]
                q = self._get_compressed(idx) if (compressed and self.compressed is not None) else None
                yield b, q if q is not None else [self._get(i) for i in idx], [[(i + 1) / self.fps, i + 1] for i in idx]
            return
        b, q, inf, count, number = 0, [], [], 0, 0
        for frame in self.frames:
            number += 1
            if self.keep is not None:
                if not self.keep(number):
                    continue
                self._kept.append(number - 1)
            count += 1
            if b % world == rank:
                self.reads += 1
                q.append(frame)
                inf.append([number / self.fps, number])
            if count % n_frames == 0:
                if q:
                    yield b, q, inf
                b, q, inf = b + 1, [], []
        self.total = count
        if q:
            yield b, q, inf

    def __iter__(self):
        """every frame of the underlying stream in order, `keep` or not (callers that sample frames themselves)"""
        if self.random_access:
            return (self._get(i) for i in range(len(self.frames)))
        return iter(self.frames)


class ExchangeLayout:
    """What one rank sends per round and how the gathered result is taken apart again; no collective, no stream.
    A face is one fp32 row of WIDTH = 517 + 2k values: 512 embedding, 4 box, 1 frame slot inside the batch [, k emotion
    class indices, k probabilities].  With world > 1 a rank's block is (cap + 1, WIDTH): a header row whose first value
    is the batch's face count, then its first `cap` faces; the others are its spill, for the follow-up gather.  With world
    == 1 nothing is gathered: the block is the payload."""

    def __init__(self, world, cap, k_emo):
        self.world, self.cap, self.k, self.WIDTH = int(world), int(cap), int(k_emo), 517 + 2 * int(k_emo)

    def payload(self, counts, boxes, emb, ticket, device):
        """a ticket's result (k > 0: and its .emo_idx / .emo_prob) as (n, WIDTH) rows on `device`; None without faces"""
        n = int(sum(counts))
        if not n:
            return None
        slot = np.repeat(np.arange(len(counts)), counts).astype(np.float32)   # frame slot inside the batch
        extra = np.concatenate([np.asarray(boxes, np.float32).reshape(n, 4), slot[:, None]], axis=1)
        cols = [emb.to(device).float(), torch.from_numpy(extra).to(device, non_blocking=True)]
        if self.k:
            if tuple(ticket.emo_idx.shape) != (n, self.k) or tuple(ticket.emo_prob.shape) != (n, self.k):
                raise ValueError("run_stream(emotions=%d): the ticket carries emotions of shape %s" % (self.k, tuple(ticket.emo_idx.shape)))
            cols += [ticket.emo_idx.to(device).float(), ticket.emo_prob.to(device).float()]
        return torch.cat(cols, dim=1)

    def cut(self, payload, device):
        """-> (the block this rank sends, the rows that did not fit or None)"""
        n = 0 if payload is None else payload.shape[0]
        if self.world == 1:
            return (payload if n else torch.empty((0, self.WIDTH), dtype=torch.float32, device=device)), None
        blk = torch.zeros((self.cap + 1, self.WIDTH), dtype=torch.float32, device=device)
        blk[0, 0] = float(n)
        if n:
            blk[1:1 + min(n, self.cap)] = payload[:self.cap]
        return blk, (payload[self.cap:] if n > self.cap else None)

    def split(self, counts, arr, more=None):
        """columns of the gathered face rows (more: and of the gathered follow-up) -> per rank r its counts[r] rows"""
        if self.world == 1:
            return [arr[:counts[0]]]
        parts = [arr[r * self.cap: r * self.cap + min(c, self.cap)] for r, c in enumerate(counts)]
        if more is not None:
            m = more.shape[0] // self.world
            parts = [np.concatenate([p, more[r * m: r * m + max(0, c - self.cap)]]) for r, (p, c) in enumerate(zip(parts, counts))]
        return parts

    def emotions(self, tail, sel):
        """the keyword that carries the emotions of the faces `sel` of the rows' tail (columns 512..); nothing without k"""
        k = self.k
        return {"emotions": (tail[sel, 5:5 + k].astype(np.int64), tail[sel, 5 + k:5 + 2 * k])} if k else {}


@dataclass
class Batch:
    """a batch between submit and its round's exchange; a rank without a batch in the last round has `rnd` only"""
    rnd: int
    ticket: object = None
    frames: object = None        # host side: arrays, or jpeg.HostFrame of a device-decoded batch
    info: object = None          # [[time, frame number], ...]
    frames_dev: object = None


@dataclass
class Round:
    """a round between its exchange and its rows; what a flag switches off stays None"""
    rnd: int
    frames: object               # this rank's batch, as in Batch; None when it ran none in this round
    info: object
    n: int = 0                   # its faces
    spill: object = None         # its device rows past `cap`
    video: object = None         # encoder: (device frames, upload slot, event they are free behind)
    hdr: object = None           # pinned host copies, valid behind `event` -- world > 1: the gathered face counts;
    extra: object = None         # classifying ranks: columns 512.. of the gathered rows, their classes and probabilities;
    amax: object = None
    prob: object = None
    emb: object = None           # face sink: columns ..512
    event: object = None


def _uploads(source, n_frames, rank, world, dev, uploader, decode, decode_entropy):
    """this rank's batches, as ((batch_index, host-side frames, info), (frames_dev, ready, slot) or None without uploader),
    the upload one batch AHEAD: submit() blocks on the detector's single read-back, so the next batch's host -> HBM copy
    has to be in flight before it, or copy and detection would take turns"""
    as_bytes = uploader is not None and decode == "device" and getattr(source, "compressed", None) is not None
    it = source.rank_batches(n_frames, rank, world, **({"compressed": True} if as_bytes else {}))

    def start(item):
        if item is None or uploader is None:
            return item, None
        from . import jpeg
        b, q, inf = item
        if isinstance(q, jpeg.CompressedBatch):
            kw = {} if decode_entropy == "host" else {"entropy": decode_entropy}
            frames_dev, ev, slot, q = jpeg.decode_batch(q, dev, uploader, **kw)
            return (b, q, inf), (frames_dev, ev, slot)
        return item, uploader.upload(q) + (uploader.last_slot,)

    nxt, up = start(next(it, None))
    while nxt is not None:
        cur, cur_up = nxt, up
        nxt, up = start(next(it, None))
        yield cur, cur_up


class _Stream:
    """One run_stream call: what its steps share.  comm / uploader are None on the CPU."""

    def __init__(self, source, pipe, n_frames, rank, world, dev, layout, comm, uploader, on_frame, encoder, row, faces):
        self.source, self.pipe, self.n_frames, self.rank, self.world, self.dev = source, pipe, n_frames, rank, world, dev
        self.layout, self.comm, self.uploader, self.on_frame, self.encoder, self.row = layout, comm, uploader, on_frame, encoder, row
        self.sink = faces if rank == 0 else None
        self.classify_here = rank == 0 or on_frame is not None or encoder is not None
        self.number_of = getattr(source, "number_of", None) or (lambda pos: pos + 1)
        self.on_comm = (lambda: torch.cuda.stream(comm)) if comm is not None else contextlib.nullcontext
        self.rows, self.pending = {}, []     # pending: issued exchanges
        self.processed, self.shape = 0, None

    def _to_host(self, x):
        if x is None or self.comm is None:
            return x
        return torch.empty(x.shape, dtype=x.dtype, pin_memory=True).copy_(x, non_blocking=True)

    def _classify(self, rows_dev):
        if not self.classify_here or rows_dev.shape[0] == 0:
            return None, None
        return self.pipe.classifier.classify(rows_dev[:, :512].contiguous(), want_logp=False)[1:3]      # (amax, prob)

    def submit(self, item, up):
        """push a batch the prefetcher yielded through the pipeline -> Batch"""
        b, q, inf = item
        if self.shape is None:
            self.shape = q[0].shape                           # frames of one stream share a shape
        if up is not None:
            frames_dev, ready, slot = up
            ticket = self.pipe.submit(frames_dev, classify=False, ready=ready)
            ticket.upload_slot = slot
        else:                                                 # CPU stand-ins: no uploader, and submit takes no `ready`
            frames_dev = self.pipe.detector._to_device_frames(q)[0]
            ticket = self.pipe.submit(frames_dev, classify=False)
        self.processed += len(q)
        return Batch(b // self.world, ticket, q, inf, frames_dev)

    def retire(self, inflight, keep=0):
        """issue the exchange of all but the `keep` newest batches in flight; consume every round but the last issued"""
        while len(inflight) > keep:
            self.pending.append(self.issue(inflight.pop(0)))
            while len(self.pending) > 1:
                self.consume(self.pending.pop(0))

    def issue(self, batch):
        """enqueue the round's exchange (+ classification of the gathered embeddings) on the side stream, behind this batch's
        own event only; nothing here waits on the host"""
        lay, dev, comm, t = self.layout, self.dev, self.comm, batch.ticket
        rec, payload = Round(batch.rnd, batch.frames, batch.info), None
        if t is not None:
            counts, boxes, emb, _, _ = t.result()
            # The batch's frames were last read by its warp, ahead of the ticket's (embedding) event (no faces: by its
            # detection, whose read-back the host has waited for): behind it the upload slot is free -- or the encoder may
            # draw on the frames, which then stay with the round; a batch outside the ring (slot -1) may be the source's own
            # tensor and is copied.  The emotions were produced ahead of that event too; result() has waited for it.
            slot, after = getattr(t, "upload_slot", -1), getattr(t, "event", None)
            if self.uploader is not None and self.encoder is None:
                self.uploader.release(slot, after)
            payload = lay.payload(counts, boxes, emb, t, dev)
            rec.n = 0 if payload is None else payload.shape[0]
            if self.encoder is not None:
                rec.video = (batch.frames_dev if slot is not None and slot >= 0 else batch.frames_dev.clone(), slot, after)
        if comm is not None:
            comm.wait_stream(torch.cuda.current_stream(dev))
        with self.on_comm():
            gathered, rec.spill = lay.cut(payload, dev)
            if self.world > 1:
                out = torch.empty((self.world * (lay.cap + 1), lay.WIDTH), dtype=torch.float32, device=dev)
                dist.all_gather_into_tensor(out, gathered)
                g = out.view(self.world, lay.cap + 1, lay.WIDTH)
                rec.hdr = self._to_host(g[:, 0, 0].contiguous())
                gathered = g[:, 1:, :].reshape(self.world * lay.cap, lay.WIDTH)
            amax, prob = self._classify(gathered)
            if self.classify_here:
                rec.extra, rec.amax, rec.prob = (self._to_host(x) for x in (gathered[:, 512:].contiguous(), amax, prob))
            if self.sink is not None:
                rec.emb = self._to_host(gathered[:, :512].contiguous())
            if payload is not None and comm is not None:
                payload.record_stream(comm)
            rec.event = comm.record_event() if comm is not None else None
        return rec

    def _follow_up(self, rec, m):
        """rare: a batch held more faces than the fixed block.  Every rank sees the same headers, so every rank issues this
        same gather of m rows per rank -> host (tail, amax, prob, emb) of its rows"""
        with self.on_comm():
            out = torch.empty((self.world * m, self.layout.WIDTH), dtype=torch.float32, device=self.dev)
            blk = torch.zeros((m, self.layout.WIDTH), dtype=torch.float32, device=self.dev)
            if rec.spill is not None:
                blk[:rec.spill.shape[0]] = rec.spill
            dist.all_gather_into_tensor(out, blk)
            amax, prob = self._classify(out)
            if self.classify_here:
                return (out[:, 512:].cpu().numpy(), amax.cpu().numpy(), prob.cpu().numpy(),
                        out[:, :512].cpu().numpy() if self.sink is not None else None)
            if self.comm is not None:
                self.comm.synchronize()
        return (None,) * 4

    def consume(self, rec):
        """host side of a round, one round after its exchange was issued: per-rank counts from the header rows, the
        follow-up gather for a batch that did not fit the fixed block, names and tracker rows"""
        if rec.event is not None:
            rec.event.synchronize()
        lay = self.layout
        counts = [rec.n] if self.world == 1 else [int(round(float(c))) for c in rec.hdr.tolist()]
        m = max(counts) - lay.cap if self.world > 1 else 0
        more = self._follow_up(rec, m) if m > 0 else (None,) * 4
        if not self.classify_here:
            return
        tails = lay.split(counts, rec.extra.numpy(), more[0])
        amax = lay.split(counts, rec.amax.numpy() if rec.amax is not None else np.zeros((0,), np.int32), more[1])
        prob = lay.split(counts, rec.prob.numpy() if rec.prob is not None else np.zeros((0,), np.float32), more[2])
        embs = lay.split(counts, rec.emb.numpy(), more[3]) if self.sink is not None else [None] * len(counts)
        amax = np.concatenate(amax)
        names = identify_names(amax, np.concatenate(prob), self.pipe.classifier.num_classes, self.pipe.label2name,
                               self.pipe.threshold) if amax.shape[0] else []
        o = 0
        for r, (tail, emb) in enumerate(zip(tails, embs)):    # rank r ran batch rnd * world + r
            nm = names[o:o + tail.shape[0]]
            o += tail.shape[0]
            if r == self.rank and rec.info is not None:
                self._collate_own(rec, nm, tail, emb)
            elif self.rank == 0:
                self._collate_other(rec.rnd * self.world + r, nm, tail, emb)

    def _frame(self, tm, num, shape, sel, nm, tail, emb, own=None):
        """a frame's callbacks in their order -- on_frame (own: my frame's pixels), row (rank 0), sink -> (names, boxes, emotions kw)"""
        f_names, f_boxes, f_emo = [nm[j] for j in sel], [tail[j, 0:4] for j in sel], self.layout.emotions(tail, sel)
        if own is not None and self.on_frame is not None:
            self.on_frame(own, num, f_names, f_boxes, **f_emo)
        if self.rank == 0:
            self.rows[num] = self.row(tm, num, f_names, f_boxes, shape, **f_emo)
        if self.sink is not None:
            for j, box in zip(sel, f_boxes):
                self.sink(num, tm, box, emb[j])
        return f_names, f_boxes, f_emo

    def _collate_own(self, rec, nm, tail, emb):
        """my own frames, one by one: pixels, times and numbers are here; then the batch goes to the encoder"""
        sl = tail[:, 4].astype(np.int64)
        b_names, b_boxes, b_emo = (list(col) for col in zip(*(
            self._frame(tm, num, rec.frames[i].shape, np.nonzero(sl == i)[0], nm, tail, emb, own=rec.frames[i])
            for i, (tm, num) in enumerate(rec.info))))
        if self.encoder is not None:
            (frames_dev, slot, after), rec.video = rec.video, None
            emo = {"emotions": [e["emotions"] for e in b_emo]} if self.layout.k else {}
            done = self.encoder.write_batch(frames_dev, [num for _, num in rec.info], b_boxes, b_names, after=after, **emo)
            self.uploader.release(slot, done)

    def _collate_other(self, batch_index, nm, tail, emb):
        """rank 0, another rank's frames, by ascending frame slot: number and time follow from the batch index"""
        sl = tail[:, 4].astype(np.int64)
        for i in np.unique(sl):
            num = self.number_of(batch_index * self.n_frames + int(i))
            self._frame(num / self.source.fps, num, self.shape, np.nonzero(sl == i)[0], nm, tail, emb)


def run_stream(source, pipe, n_frames, rank=0, world=1, device=None, on_frame=None, log=None, lag=2, cap=None,
               decode="device", encoder=None, emotions=0, row=None, decode_entropy="host", faces=None):
    """Push this rank's batches through `pipe.submit`, exchange per round, collate on rank 0.

    pipe: FacePipeline-like -- .submit(frames_dev, classify=False[, ready=event]) -> ticket with .result() ->
    (counts, boxes (n,4) host, emb (n,512) device, _, _), .flush(), .detector._to_device_frames(list) (CPU stand-ins
    only; on a GPU the frames go through upload.FrameUploader), .classifier.classify(emb, want_logp=False) ->
    (_, amax, prob), .classifier.num_classes, .label2name, .threshold.
    on_frame(frame_rgb, frame_number, names, boxes): called on the rank that owns the frame (annotated-frame writer);
    requesting it makes every rank classify the gathered embeddings (the names are needed where the pixels are).
    cap: faces per rank and round carried by the fixed-size exchange (default max(256, 16 * n_frames)).
    decode: "device" (default) -- on a GPU, a batch the source can hand over as JPEG bytes (FrameSource.compressed) is
    decoded by jpeg.decode_batch_device: entropy decode on host threads, pixels on the upload stream; a batch it does
    not take is decoded by Pillow and uploaded, as every batch is with decode="host".  The frames are the same bytes
    either way; on_frame receives a jpeg.HostFrame (shape + pixels on demand) for a device-decoded frame.
    decode_entropy: "host" (default) or "device" -- where the Huffman decode of such a batch runs (jpeg.ENTROPY): on
    host threads, or in HIP behind an upload of the compressed frames as they are.  Ignored with decode="host".
    encoder: None, or a jpeg_encode.VideoEncoder-like object (GPU only) that writes the annotated video: every batch's
    DEVICE frames are then kept until the round's names are known and handed over with
    .write_batch(frames_dev, numbers, boxes, names, after=event) -> event, in frame order on the rank that owns them;
    it draws on them in place (frames without faces go through unannotated; a batch that is not a slot of the upload
    ring -- a source that hands out cuda tensors -- is copied first, the source's frames are never painted).  Like on_frame it makes every rank
    classify.  The batch's slot of the upload ring is released behind the encoder's event, not the embedding's.
    emotions: k > 0 (at most 16, vnf_softmax_topk's limit) makes the exchange carry every face's top-k emotions: the
    tickets then have .emo_idx / .emo_prob ((n,k), FacePipeline(emotion=...)), a row of the block is 517 + 2k fp32
    values -- the k class indices as fp32 (exact below 2^24 classes; a pipe whose .emotion.num_classes is not refused),
    then the k probabilities --, and on_frame, encoder.write_batch and `row` receive the keyword
    emotions=(idx (n,k) int64, prob (n,k) fp32) per frame (write_batch: a list of them).  k is the same on every
    rank (a CLI flag): the block's width follows from it alone.  0 (default): nothing of this, tickets need no emo_*.
    row: the tracker line's formatter, (time, frame_number, names, boxes, frame_shape[, emotions=...]) -> str; default
    `tracker_row`.
    faces: None (default: nothing below happens), or a callable that rank 0 hands every face of every round, in the order
    the tracker rows list them: faces(frame_number, time, box (4,) fp32, embedding (512,) host fp32) -- the gathered
    embeddings as they were exchanged, for rank 0's own frames and for the other ranks' alike (tracking.py links them
    into tracks after the stream).  It costs one more pinned read-back per round, of gathered[:, :512], on rank 0 only;
    the collectives and the rows are the same with and without it.
    Returns (rows: {frame_number: csv row}, complete on rank 0; frames processed by this rank)."""
    k_emo = int(emotions)
    if not 0 <= k_emo <= 16:
        raise ValueError("run_stream: emotions must be in 0..16, got %r" % (emotions,))
    if k_emo and int(getattr(getattr(pipe, "emotion", None), "num_classes", 0) or 0) >= 1 << 24:
        raise ValueError("run_stream: the exchange carries emotion indices as fp32, exact below 2^24 classes only")
    for name, value, ok in (("decode", decode, ("device", "host")), ("decode_entropy", decode_entropy, ("host", "device"))):
        if value not in ok:
            raise ValueError("run_stream: %s must be %r or %r, got %r" % (name, ok[0], ok[1], value))
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    comm = uploader = None
    if dev.type == "cuda":
        from .streams import side_stream
        from .upload import FrameUploader
        comm = side_stream(dev, 7)          # the collective's stream (roles 0..6 belong to the pipeline, streams.py)
        uploader = FrameUploader(dev, depth=lag + 3 + (2 if encoder is not None else 0))
    elif encoder is not None:
        raise RuntimeError("run_stream: the video encoder works on frames in device memory (there is no CPU path)")
    layout = ExchangeLayout(world, int(cap) if cap else max(256, 16 * int(n_frames)), k_emo)
    st = _Stream(source, pipe, n_frames, rank, world, dev, layout, comm, uploader, on_frame, encoder, row or tracker_row, faces)
    inflight, rounds = [], 0                # submitted batches, retired `lag` late; rounds this rank has a batch in
    for item, up in _uploads(source, n_frames, rank, world, dev, uploader, decode, decode_entropy):
        inflight.append(st.submit(item, up))
        rounds = inflight[-1].rnd + 1
        if log is not None:
            log(st.processed, item[2])
        st.retire(inflight, lag)
    # Every rank joins every round's exchange, in round order, and issues no other collective: it knows the stream's length
    # by now (random access: len(); a decoder: it has pulled every frame).  It owns rounds 0 .. rounds-1; only the last may be missing.
    total_frames = int(source.total if source.total is not None else st.processed)
    total_rounds = ((total_frames + n_frames - 1) // n_frames + world - 1) // world
    inflight += [Batch(rnd) for rnd in range(rounds, total_rounds)]
    if hasattr(pipe, "flush"):
        pipe.flush()
    st.retire(inflight)
    for rec in st.pending:                  # the last round issued, if there was any
        st.consume(rec)
    if uploader is not None:
        uploader.close()
    if rank == 0:
        # a frame without faces sent nothing through the exchange: its (empty) row follows from the frame count
        none = layout.emotions(np.zeros((0, layout.WIDTH - 512), np.float32), np.zeros((0,), np.int64))
        for num in (st.number_of(pos) for pos in range(total_frames)):
            if num not in st.rows:
                st.rows[num] = st.row(num / source.fps, num, [], [], st.shape or (1, 1, 3), **none)
    return st.rows, st.processed
