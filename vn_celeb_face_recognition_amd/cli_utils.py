"""Small host helpers the CLIs share (formats kept from the reference):
  read_json, start_tracker's header line (append_log_to_file)      <- /root/reference/utils/utils.py:34-38,60-64 (77-82: statistics.py)
  label2name CSV ('label,name' header)                             <- demo_image.py:359, meta_data/face_recognition/label2name.txt
  draw_boxes_on_image                                              <- demo_image.py:150-158 (PIL instead of OpenCV, which is not installed)
  draw_emotions                                                    <- demo_image.py:161-171 (text only, drawn the same way)
  load_etag2idx                                                    <- utils/utils.py load_pickle on meta_data/emotion_recognition/etag2idx.pkl.keep
"""
import contextlib
import csv
import glob
import json
import os
import time

import numpy as np
from PIL import Image, ImageDraw

try:
    import cv2
except ImportError:
    cv2 = None                   # no OpenCV: video goes in and out as Motion-JPEG .avi only

from .statistics import convert_sec_to_max_time_quantity  # noqa: F401  (one definition; part of this module's surface)


def read_json(filename):
    with open(filename, 'r') as fp:
        return json.load(fp)


def read_label2name(path):
    """CSV with header label,name -> {'label': [...], 'name': [...]} (column access like the DataFrame)."""
    labels, names = [], []
    with open(path, newline='') as f:
        for row in csv.DictReader(f):
            labels.append(int(row['label']))
            names.append(row['name'])
    return {'label': labels, 'name': names}


def read_rgb(path):
    return np.asarray(Image.open(path).convert('RGB'))


def write_rgb(path, rgb):
    Image.fromarray(np.asarray(rgb, dtype=np.uint8)).save(path)


def draw_boxes_on_image(rgb_image, boxes, list_names):
    """Green 2-px rectangles with the name at the top-right corner (demo_image.py:150-158)."""
    im = Image.fromarray(np.asarray(rgb_image, dtype=np.uint8).copy())
    d = ImageDraw.Draw(im)
    for box, name in zip(boxes, list_names):
        d.rectangle([float(box[0]), float(box[1]), float(box[2]), float(box[3])], outline=(0, 255, 0), width=2)
        d.text((float(box[2]), float(box[1])), str(name), fill=(0, 255, 0))
    return np.asarray(im)


def draw_emotions(rgb_image, bboxes, emotion_tags, emotion_percent):
    """'<tag> - <percent>%' lines inside each box, 16 px apart from its top-left corner (demo_image.py:161-171)."""
    im = Image.fromarray(np.asarray(rgb_image, dtype=np.uint8).copy())
    d = ImageDraw.Draw(im)
    for idx, box in enumerate(bboxes):
        for i, (emotion, percent) in enumerate(zip(emotion_tags[idx], emotion_percent[idx])):
            d.text((int(box[0] + 5), int(box[1]) + i * 16 + 4), '{} - {:.2f}%'.format(emotion, percent * 100), fill=(0, 255, 0))
    return np.asarray(im)


def load_etag2idx(path):
    """The emotion tag table {'key2idx': {tag: index}, 'idx2key': {index: tag}} (demo_image.py:380).  A .json file of
    that shape (idx2key as a list or a dict, key2idx optional) or the reference's pickle, which is read by an
    unpickler that admits builtin containers, str and int only: a pickle that names any global is refused."""
    import io
    import pickle
    if str(path).lower().endswith('.json'):
        tab = read_json(path)
    else:
        class _Restricted(pickle.Unpickler):
            def find_class(self, module, name):
                raise pickle.UnpicklingError("etag2idx pickle names the global %s.%s: only builtin containers, str and "
                                             "int are admitted" % (module, name))
        with open(path, 'rb') as f:
            tab = _Restricted(io.BytesIO(f.read())).load()

    def plain(x):
        return isinstance(x, (str, int)) and not isinstance(x, bool)
    if not isinstance(tab, dict) or 'idx2key' not in tab:
        raise ValueError("%s: expected a dict with 'idx2key'" % (path,))
    i2k = tab['idx2key']
    if isinstance(i2k, (list, tuple)):
        i2k = dict(enumerate(i2k))
    if not isinstance(i2k, dict) or not all(plain(k) and plain(v) for k, v in i2k.items()):
        raise ValueError("%s: idx2key must map int -> str" % (path,))
    idx2key = {int(k): str(v) for k, v in i2k.items()}
    k2i = tab.get('key2idx')
    if k2i is None:
        key2idx = {v: k for k, v in idx2key.items()}
    else:
        if not isinstance(k2i, dict) or not all(plain(k) and plain(v) for k, v in k2i.items()):
            raise ValueError("%s: key2idx must map str -> int" % (path,))
        key2idx = {str(k): int(v) for k, v in k2i.items()}
    return {'key2idx': key2idx, 'idx2key': idx2key}


def export_video_face_recognition(output_frame_dir, fps, output_path):
    """demo_video.py:25-43: frame_1.png .. frame_N.png of the output directory -> one video.  cv2.VideoWriter (MP4V) when
    OpenCV is importable; otherwise a Motion-JPEG AVI (output_path must end in .avi)."""
    n_images = len(glob.glob(os.path.join(output_frame_dir, '*')))
    paths = [os.path.join(output_frame_dir, 'frame_{}.png'.format(i)) for i in range(1, n_images + 1)]
    paths = [p for p in paths if os.path.exists(p)]
    if not paths:
        raise RuntimeError("export_video_face_recognition: no frame_<i>.png under %r (run with -sfr)" % output_frame_dir)
    if cv2 is not None:
        first = cv2.imread(paths[0])
        out_writer = cv2.VideoWriter(output_path, cv2.VideoWriter_fourcc(*'MP4V'), fps, (first.shape[1], first.shape[0]))
        for pth in paths:
            out_writer.write(cv2.imread(pth))
        out_writer.release()
    else:
        if not output_path.lower().endswith('.avi'):
            raise RuntimeError("without OpenCV the exported video is a Motion-JPEG AVI: give -ov a name ending in .avi")
        from .mjpeg_avi import write_mjpeg_avi
        write_mjpeg_avi(output_path, (read_rgb(pth) for pth in paths), fps)
    print('Save exported video in {} ...'.format(output_path))


def add_stream_arguments(p, fps_default, fps_help=None, ov_help=None, ov='-ov'):
    """the stream flags demo_video.py and celeb_statistic.py share; `ov`: what their help texts call the device-encoded video"""
    p.add_argument('-i', '--video_path', default='video.mp4', type=str)
    p.add_argument('-o', '--output_frame', default='output_frame', type=str)
    p.add_argument('-ot', '--output_tracker', default='tracker.csv', type=str)
    p.add_argument('-sfr', '--save_frame_recognized', action='store_true')
    p.add_argument('--log_step', default=100, type=int)
    p.add_argument('--n_frames', default=16, type=int)
    p.add_argument('-fps', '--fps_video', default=fps_default, type=float, help=fps_help)
    p.add_argument('--host_decode', action='store_true',
                   help='decode JPEG frames (Motion-JPEG .avi, .jpg directory) with Pillow on the host instead of on the GPU')
    p.add_argument('--decode_entropy', default='host', choices=['host', 'device'],
                   help='where the Huffman decode of JPEG frames decoded on the GPU runs: on host threads, or on the GPU too '
                        '(the compressed frames are uploaded as they are; the same pixels); ignored with --host_decode')
    p.add_argument('-ov', '--output_video', default='', type=str, help=ov_help)
    p.add_argument('--ov_quality', default=92, type=int, help='JPEG quality of the frames of {} (1..100)'.format(ov))
    p.add_argument('--ov_subsampling', default='4:2:0', choices=['4:4:4', '4:2:2', '4:2:0'],
                   help='chroma subsampling of the frames of {}'.format(ov))
    p.add_argument('--ov_entropy', default='host', choices=['host', 'device'],
                   help='where the Huffman pass of the frames of {} runs: on host threads, or on the GPU (the same files)'.format(ov))


def start_tracker(args, header):
    """rank 0, before the stream: the frame directory, and a tracker file that holds the header line only"""
    os.makedirs(args.output_frame, exist_ok=True)
    with open(args.output_tracker, 'w') as f:
        f.write(','.join(header) + '\n')


def progress_log(log_step):
    """run_stream's `log`: a console line whenever this rank's frame count reaches a multiple of --log_step"""
    def log(processed, inf):
        if (processed % log_step) == 0:
            print('Processing for frame: {}, time: {}'.format(inf[-1][1], convert_sec_to_max_time_quantity(inf[-1][0])))
    return log


def total_processed(processed, world, device):
    """the frames all ranks processed: with world > 1 one all_reduce, which every rank issues"""
    if world > 1:
        import torch
        tot = torch.tensor([processed], device=device if device is not None else 'cuda')
        torch.distributed.all_reduce(tot)
        processed = int(tot.item())
    return processed


def finish_tracker(path, rows, processed, start_time):
    """rank 0, after the stream: the rows in frame order behind the header, and the two closing console lines"""
    with open(path, 'a') as f:
        f.write(''.join(rows[k] for k in sorted(rows)))
    print('Saved tracker file in {} ...'.format(path))
    print('FPS for recognition face: {}'.format(int(processed / max(time.time() - start_time, 1e-9))))


@contextlib.contextmanager
def video_export(args, on, fps, device, rank, world, idx2tag=None):
    """`with` around a run: -ov's jpeg_encode.VideoEncoder when `on`, else None.  An exception in the run aborts it (no half-
    written video, no spool file); else it is closed, the ranks wait for each other's spool files and rank 0 merges them."""
    if not on:
        yield None
        return
    from .jpeg_encode import VideoEncoder
    encoder = VideoEncoder(args.output_video, fps, device, args.ov_quality, args.ov_subsampling, rank, world, idx2tag=idx2tag,
                           entropy=args.ov_entropy)
    try:
        yield encoder
    except BaseException:
        encoder.abort()
        raise
    try:
        encoder.close()
    except ValueError as e:                                   # a stream without (sampled) frames
        raise SystemExit("-ov: {}".format(e))
    if world > 1:
        import torch
        torch.distributed.barrier()
        if rank == 0:
            encoder.merge()
    if rank == 0:
        print('Save exported video in {} ...'.format(args.output_video))


def open_frame_source(path):
    """video.FrameSource over RGB frames.  Accepts a directory of images (sorted; random access: a rank decodes only its
    own batches), a .npy/.npz array of (T,H,W,3) uint8 frames (memory-mapped), a Motion-JPEG .avi (pure-Python RIFF
    walker, mjpeg_avi.py), or any video file when OpenCV is importable (demo_video.py:78-81; sequential: the other
    ranks' frames are decoded and dropped)."""
    from .video import FrameSource
    if os.path.isdir(path):
        files = sorted(f for f in os.listdir(path) if f.lower().endswith(('.png', '.jpg', '.jpeg', '.bmp')))
        paths = [os.path.join(path, f) for f in files]

        def jpeg_bytes(i):
            if not paths[i].lower().endswith(('.jpg', '.jpeg')):
                return None
            with open(paths[i], 'rb') as f:
                return f.read()
        return FrameSource(paths, 25.0, load=read_rgb, compressed=jpeg_bytes)
    if path.endswith('.npy'):
        return FrameSource(np.load(path, mmap_mode='r'), 30.0)
    if path.endswith('.npz'):
        return FrameSource(np.load(path)['arr_0'], 30.0)
    if cv2 is None:
        from .mjpeg_avi import read_mjpeg_avi
        try:
            fps, frames, _ = read_mjpeg_avi(path)
        except (ValueError, OSError) as e:
            raise RuntimeError("decoding %r needs OpenCV, which is not installed (%s): pass a Motion-JPEG .avi, a directory "
                               "of frames or a .npy array of (T,H,W,3) uint8 RGB frames instead" % (path, e))
        return FrameSource(frames, fps, compressed=frames.compressed)
    cap = cv2.VideoCapture(path)
    fps = cap.get(cv2.CAP_PROP_FPS) or 25.0

    def gen():
        while cap.isOpened():
            ret, frame = cap.read()
            if not ret:
                break
            yield frame[:, :, ::-1]
        cap.release()
    return FrameSource(gen(), fps)
