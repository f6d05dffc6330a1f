#!/usr/bin/env python3
"""Celebrity statistics over a frame stream: drop-in for /root/reference/celeb_statistic.py.

Same flags and files: frames are sub-sampled per second of video with -fidx (l.180-187), queued in batches of
--n_frames, recognised with per-class thresholds (--local_thresholds JSON, or --recog_threshold for every class,
l.127-136), logged to the tracker CSV (Time,Names,Frame_idx[,Bboxes][,Emotion], l.137-147,253-276; an existing tracker
file is re-used, l.393-399) and summarised into the interval JSON (`dynamic_itv` / `fixed_itv`, l.32-107, 401-412).

The frames go through video.run_stream, the path demo_video.py runs on: launched under torch.distributed.run, batch b
of the SAMPLED frames belongs to -- and is read by -- rank b % world_size only, the ranks all-gather embeddings, boxes
and emotions per round and rank 0 writes the tracker and the statistics.  Only the frames -fidx keeps are read and
decoded (a directory, a .npy array, a Motion-JPEG .avi; JPEG frames on the GPU unless --host_decode, their Huffman decode there too with
--decode_entropy device); frame number and
time stay those of the input.  --recog_emotion (-emt, -emtargs, -t2i, --topk_emotions) adds every face's top-k emotion
tags to the tracker (column Emotion, l.264-271) and to the 'emotions' field of the JSON, the mode the reference's own
scripts run (scripts/celeb_stat_*.sh).  -sfr writes the annotated PNGs (boxes, names, emotion lines) on the host;
-ov out.avi writes the annotated video of the sampled frames from the device (jpeg_encode.VideoEncoder: boxes, names
and emotion lines drawn in HBM, --ov_quality, --ov_subsampling; --ov_entropy device runs the Huffman pass of the
encoder in HIP too, the same files, default host) at as many frames per second as -fidx keeps, so the
video lasts as long as the input.  --track_faces (--track_threshold, --track_iou, --track_gap; this build's, the
reference names every face on its own) links the faces of consecutive processed frames into tracks on the GPU after the
stream (tracking.py, csrc/gallery_tracks.hip) and writes every face under its track's name, with a last tracker column
Track; it is refused together with -ov and -sfr, which draw the names while the frames pass.  Input: a directory of frames or a .npy array of (T,H,W,3) RGB frames with -fps, or
a Motion-JPEG .avi (OpenCV / pafy are not installed: no other container decode, no YouTube); seq_fd_vs_aln (outside
the hot path) is refused."""
import os
import time

import numpy as np
import torch
import torch.distributed as dist

from demo_image import build_emotion, build_models, build_parser
from vn_celeb_face_recognition_amd import dist as vdist
from vn_celeb_face_recognition_amd.cli_utils import (add_stream_arguments, draw_boxes_on_image, draw_emotions, finish_tracker,
                                                     open_frame_source, progress_log, start_tracker, total_processed,
                                                     video_export, write_rgb)
from vn_celeb_face_recognition_amd.pipeline import FacePipeline
from vn_celeb_face_recognition_amd.statistics import (build_thresholds, export_json_stat_dynamic_itv, export_json_stat_fixed_itv,
                                                      frame_is_sampled, read_tracker_csv, tracker_header, tracker_row)
from vn_celeb_face_recognition_amd.video import run_stream


def emotion_tags(idx2etag, idx):
    """celeb_statistic.py:264-271: per face the plain-str list of its top-k tags ([] for a frame without faces)"""
    return [[str(idx2etag[int(i)]) for i in face] for face in idx]


def sampled_source(args, frame_idxes):
    """the frame source reduced to the frames -fidx keeps (celeb_statistic.py:180-187) -> (source, kept frames per second of input)"""
    source = open_frame_source(args.video_path)
    if args.fps_video > 0:
        source.fps = float(args.fps_video)
    fps = source.fps
    source.sample(lambda count: frame_is_sampled(count, fps, frame_idxes))
    # count % fps takes every value below fps once per second of video (an integral rate; otherwise about once)
    kept = len({i for i in frame_idxes if 0 <= i < fps})
    return source, kept


def main(args, pipe, rank, world, source, device=None, encoder=None, idx2etag=None):
    """celeb_statistic.py:150-300 on video.run_stream; identical control flow for every world size"""
    k = args.topk_emotions if idx2etag is not None else 0
    if rank == 0:
        start_tracker(args, tracker_header(args.track_bbox, k > 0, args.track_faces))
    start_time = time.time()
    frames_seen, faces_seen = {}, []           # --track_faces, rank 0: what every row was made of; every face of the stream

    def row(tm, number, names, boxes, shape, emotions=None, tracks=None):
        if args.track_faces and tracks is None:
            frames_seen[number] = (tm, boxes, shape, emotions)
        return tracker_row(tm, names, number, boxes, shape[:2], args.track_bbox,
                           emotion_tags(idx2etag, emotions[0]) if emotions is not None else None, tracks)

    def face(number, tm, box, emb):
        faces_seen.append((number, np.array(emb, np.float32), np.array(box, np.float32)))

    def on_frame(frame, number, names, boxes, emotions=None):
        img = draw_boxes_on_image(frame, boxes, names) if names else frame
        if names and emotions is not None:
            img = draw_emotions(img, boxes, emotion_tags(idx2etag, emotions[0]), emotions[1])
        write_rgb(os.path.join(args.output_frame, 'frame_{}.png'.format(number)), img)

    rows, processed = run_stream(source, pipe, args.n_frames, rank, world, device=device,
                                 on_frame=on_frame if args.save_frame_recognized else None, log=progress_log(args.log_step),
                                 decode="host" if args.host_decode else "device", encoder=encoder, emotions=k, row=row,
                                 decode_entropy=args.decode_entropy, faces=face if args.track_faces else None)
    processed = total_processed(processed, world, device)
    if rank != 0:
        return None
    if args.track_faces:
        rows = track_rows(args, pipe, device, frames_seen, faces_seen, row)
    finish_tracker(args.output_tracker, rows, processed, start_time)
    return read_tracker_csv(args.output_tracker)


def track_rows(args, pipe, device, frames_seen, faces_seen, row):
    """--track_faces, after the stream: the faces in frame order (the order of their tracker row within a frame), linked
    into tracks and named per track (tracking.py) -> the tracker rows again, every face under its track's name, with the
    track ids of the row's faces for a last column."""
    from vn_celeb_face_recognition_amd.tracking import link_tracks, name_tracks, pool_tracks
    numbers = sorted(frames_seen)
    ordinal = {num: p for p, num in enumerate(numbers)}      # a frame's position among the processed frames
    order = sorted(range(len(faces_seen)), key=lambda i: faces_seen[i][0])   # stable: the stream's order inside a frame
    emb = np.stack([faces_seen[i][1] for i in order]) if order else np.zeros((0, 512), np.float32)
    boxes = np.stack([faces_seen[i][2] for i in order]) if order else np.zeros((0, 4), np.float32)
    frame_ord = np.array([ordinal[faces_seen[i][0]] for i in order], np.int64)
    res = link_tracks(emb, frame_ord, boxes, threshold=args.track_threshold, min_iou=args.track_iou, max_gap=args.track_gap,
                      device=device)
    names = name_tracks(pool_tracks(emb, res), pipe.classifier, pipe.label2name, pipe.threshold)
    print('Linked {} faces into {} tracks'.format(len(order), res.n_tracks))
    rows, o = {}, 0
    for num in numbers:
        tm, f_boxes, shape, emotions = frames_seen[num]
        ids = res.track[o:o + len(f_boxes)].tolist()
        assert (frame_ord[o:o + len(f_boxes)] == ordinal[num]).all()
        o += len(f_boxes)
        kw = {} if emotions is None else {"emotions": emotions}
        rows[num] = row(tm, num, [names[t] for t in ids], f_boxes, shape, tracks=ids, **kw)
    return rows


def make_parser():
    """the command line of this script"""
    p = build_parser('Face recognition on a video')
    add_stream_arguments(p, fps_default=0.0, fps_help='frame rate of a frame directory / .npy input',
                         ov_help='annotated video of the sampled frames, encoded on the GPU (Motion-JPEG .avi)')
    p.add_argument('-jst', '--json_tracker', default='tracker.json', type=str)
    p.add_argument('-fidx', '--frame_idxes', nargs='+', type=int, required=True)
    p.add_argument('-ign', '--ignored_name', default='Unknown', type=str)
    p.add_argument('-nvi', '--n_video_intervals', default=5, type=int)
    p.add_argument('-tap', '--n_time_appear', default=8, type=int)
    p.add_argument('--statistic_mode', default='dynamic_itv', type=str, help='dynamic_itv or fixed_itv')
    p.add_argument('--time_an_interval', default=5, type=int)
    p.add_argument('--local_thresholds', default='', type=str)
    p.add_argument('--track_bbox', action='store_true')
    p.add_argument('--youtube_video', action='store_true')
    p.add_argument('--track_faces', action='store_true',
                   help='link the faces of consecutive processed frames into tracks on the GPU and name every face by its '
                        'track: one name per track, decided from all of its frames; adds the column Track to the tracker')
    p.add_argument('--track_threshold', default=None, type=float,
                   help='cosine two faces of one track must reach: required with --track_faces, no default -- the threshold '
                        'calibrate.py prints for the encoder in use')
    p.add_argument('--track_iou', default=0.0, type=float,
                   help='with --track_faces: the IoU the boxes of two linked faces must reach; 0 (default) ignores the boxes. '
                        'The default is a convention, not a measurement')
    p.add_argument('--track_gap', default=1, type=int,
                   help='with --track_faces: how many processed frames a link may span (1..255); 1 (default) links adjacent '
                        'processed frames only.  The default is a convention, not a measurement')
    p.set_defaults(recog_threshold=0.7)          # celeb_statistic.py:349 (demo_image's default is 0)
    return p


if __name__ == '__main__':
    p = make_parser()
    args = p.parse_args()
    if args.youtube_video:
        raise SystemExit("--youtube_video needs pafy and network access, neither of which this build has")
    if args.inference_method != 'par_fd_vs_aln':
        raise SystemExit("use --inference_method par_fd_vs_aln (seq_fd_vs_aln needs the FAN landmark network, outside "
                         "the hot path and broken in the reference for list input)")
    if args.output_video and not args.output_video.lower().endswith('.avi'):
        raise SystemExit("-ov encodes the annotated frames on the GPU into a Motion-JPEG AVI: give it a name ending in .avi")
    if args.output_video and not 1 <= args.ov_quality <= 100:
        raise SystemExit("--ov_quality must be in 1..100")
    if args.recog_emotion and not 1 <= args.topk_emotions <= 16:
        raise SystemExit("--topk_emotions must be in 1..16 (the width of the device top-k and of the stream's exchange)")
    if args.track_faces:
        if args.track_threshold is None or args.track_threshold != args.track_threshold:
            p.error("--track_faces needs --track_threshold (a cosine: the value calibrate.py prints)")
        if not 1 <= args.track_gap <= 255:
            p.error("--track_gap must be in 1..255")
        if args.output_video or args.save_frame_recognized:
            raise SystemExit("--track_faces knows the names only after the stream: it cannot be combined with -ov or -sfr, which "
                             "draw them while the frames pass (a second pass over the frames is not implemented)")
    frame_idxes = list(args.frame_idxes)
    rank, world, local = vdist.init_from_env()
    # one decision for every rank: the tracker file appears while rank 0 works, so a late rank must not look for it
    create = not os.path.exists(args.output_tracker)
    if world > 1:
        flag = [create]
        dist.broadcast_object_list(flag, src=0, device=torch.device('cuda', local))
        create = flag[0]
    tracker_df = None
    if create:
        if rank == 0:
            print('Create tracker file {}'.format(args.output_tracker))
        device = 'cuda:%d' % local
        torch.cuda.set_device(local)
        label2name_df, detection_md, emb_model, classify_model = build_models(args, device, allow_emotion=True)
        idx2etag = emt_model = None
        if args.recog_emotion:
            idx2etag, emt_model = build_emotion(args, device)
        if args.local_thresholds != '':
            print('Using local thresholds !')
        else:
            print('Using global a threshold !')
        threshold = build_thresholds(args.local_thresholds, args.num_classes, args.recog_threshold)
        pipe = FacePipeline(detection_md, emb_model, classify_model, label2name_df, args.target_face_size, threshold,
                            embed_batch=256, emotion=emt_model, topk_emotions=args.topk_emotions)
        source, kept_per_second = sampled_source(args, frame_idxes)
        with video_export(args, bool(args.output_video), float(max(kept_per_second, 1)), device, rank, world, idx2etag) as encoder:
            tracker_df = main(args, pipe, rank, world, source, device=device, encoder=encoder, idx2etag=idx2etag)
    elif rank == 0:
        print('Re-use tracker file {}'.format(args.output_tracker))
        tracker_df = read_tracker_csv(args.output_tracker)
    if world > 1:
        dist.destroy_process_group()
    if rank != 0:
        raise SystemExit(0)
    print('Statistic mode: {}'.format(args.statistic_mode))
    if not args.track_bbox and 'Bboxes' not in tracker_df:
        raise SystemExit("the interval statistics need the Bboxes column: run with --track_bbox (the reference raises "
                         "KeyError here, celeb_statistic.py:81-82)")
    if args.statistic_mode == 'dynamic_itv':
        export_json_stat_dynamic_itv(tracker_df, args.json_tracker, args.n_video_intervals, args.n_time_appear,
                                     args.ignored_name)
    elif args.statistic_mode == 'fixed_itv':
        n_rows_in_itv = args.time_an_interval * len(frame_idxes) * 60
        export_json_stat_fixed_itv(tracker_df, args.json_tracker, n_rows_in_itv, args.n_time_appear, args.ignored_name)
    else:
        print('This statistic mode {} is not supported !'.format(args.statistic_mode))
