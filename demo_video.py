#!/usr/bin/env python3
"""Face recognition on a frame stream: drop-in for /root/reference/demo_video.py (main 46-199, CLI
202-287): same flags, tracker CSV (header Time,Names,Frame_idx,Bboxes; rows 155-168) and console lines.

Each queue of --n_frames frames goes through the resident throughput pipeline (FacePipeline.submit: detect ->
align -> embed in HBM, detection and embedding streams overlapped).  Launched under torch.distributed.run,
frame batch b is handled -- and read -- by rank b % world_size only (frames are independent,
demo_video.py:186-188); per round the ranks all-gather their embeddings + boxes over RCCL on a side stream
and rank 0 classifies the gathered tensor and writes the tracker rows in frame order (video.run_stream).
Annotated frames are written only with -sfr (the reference's test at l.149 is always true and
PNG-encodes every frame).  Input: a directory of frames, a .npy array of
(T,H,W,3) RGB frames, a Motion-JPEG .avi, or any video file when OpenCV is installed; -ov exports the annotated frames
as a video (MP4V with OpenCV, Motion-JPEG .avi without).  JPEG frames (a Motion-JPEG .avi, .jpg files) are decoded on the
GPU (jpeg.py: Huffman decode on host threads, IDCT / upsampling / colour in HIP), bit-exact to the host decoder;
--host_decode keeps them on Pillow; --decode_entropy device moves the Huffman decode into HIP as well (the compressed frames
are uploaded as they are; the same pixels; default host).  -ov x.avi WITHOUT -sfr never makes a PNG: boxes and names are drawn on the frames
where they lie in HBM and the frames are JPEG-encoded there (jpeg_encode.py: overlay, colour, down-sampling, DCT and
quantisation in HIP, the Huffman pass on host threads), the same files Pillow would write (--ov_quality,
--ov_subsampling).  --ov_entropy device runs the Huffman pass in HIP as well (the same files; only they cross to the
host, not the coefficients); the default is host."""
import os
import time

import torch
import torch.distributed as dist

from demo_image import build_models, build_parser
from vn_celeb_face_recognition_amd import dist as vdist
from vn_celeb_face_recognition_amd.cli_utils import (add_stream_arguments, draw_boxes_on_image, export_video_face_recognition,
                                                     finish_tracker, open_frame_source, progress_log, start_tracker,
                                                     total_processed, video_export, write_rgb)
from vn_celeb_face_recognition_amd.pipeline import FacePipeline
from vn_celeb_face_recognition_amd.video import run_stream, tracker_row  # noqa: F401  (tracker_row: part of this module's surface)


def main(args, pipe, rank, world, source=None, device=None, encoder=None):
    """demo_video.py:46-199 on the resident pipeline; identical control flow for every world size (video.run_stream).
    encoder: a jpeg_encode.VideoEncoder that receives every annotated frame (-ov without -sfr), or None."""
    if rank == 0:
        start_tracker(args, ['Time', 'Names', 'Frame_idx', 'Bboxes'])
    print('Method: {}'.format(args.inference_method))
    if source is None:
        source = open_frame_source(args.video_path)
    start_time = time.time()

    def on_frame(frame, number, names, boxes):
        img = draw_boxes_on_image(frame, boxes, names) if names else frame
        write_rgb(os.path.join(args.output_frame, 'frame_{}.png'.format(number)), img)

    rows, processed = run_stream(source, pipe, args.n_frames, rank, world, device=device, log=progress_log(args.log_step),
                                 on_frame=on_frame if args.save_frame_recognized else None, encoder=encoder,
                                 decode="host" if args.host_decode else "device", decode_entropy=args.decode_entropy)
    processed = total_processed(processed, world, device)
    if rank == 0:
        finish_tracker(args.output_tracker, rows, processed, start_time)


def make_parser():
    """the command line of this script"""
    p = build_parser('Face recognition on a video')
    add_stream_arguments(p, fps_default=25.0, ov='-ov without -sfr')
    return p


if __name__ == '__main__':
    args = make_parser().parse_args()
    if args.inference_method != 'par_fd_vs_aln':
        raise SystemExit("use --inference_method par_fd_vs_aln (seq_fd_vs_aln needs the FAN landmark network, outside "
                         "the hot path and broken in the reference for list input)")
    device_video = bool(args.output_video) and not args.save_frame_recognized
    if device_video and not args.output_video.lower().endswith('.avi'):
        raise SystemExit("-ov without -sfr encodes the annotated frames on the GPU into a Motion-JPEG AVI: give -ov a name "
                         "ending in .avi, or add -sfr to assemble the PNGs of --output_frame on the host")
    if device_video and not 1 <= args.ov_quality <= 100:
        raise SystemExit("--ov_quality must be in 1..100")
    rank, world, local = vdist.init_from_env()
    device = 'cuda:%d' % local
    torch.cuda.set_device(local)
    label2name_df, detection_md, emb_model, classify_model = build_models(args, device)
    pipe = FacePipeline(detection_md, emb_model, classify_model, label2name_df, args.target_face_size, args.recog_threshold,
                        embed_batch=256)
    with video_export(args, device_video, args.fps_video, device, rank, world) as encoder:
        main(args, pipe, rank, world, device=device, encoder=encoder)
    if not device_video and args.output_video and rank == 0:
        export_video_face_recognition(args.output_frame, args.fps_video, args.output_video)     # demo_video.py:285-287
    if world > 1:
        dist.destroy_process_group()
