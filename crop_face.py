#!/usr/bin/env python3
"""Cut the first detected face out of every picture of a directory: drop-in for /root/reference/crop_face.py.
Same flags; the detector is resolved by name from JSON kwargs (75-78) and runs on the GPU.  Per file (20-49): skipped if
the output exists; without a box the path goes to the unknown file; with more than one box the path goes to the
many-boxes file and box 0 is still cropped; the crop is [max(int(y1),0):min(int(y2+1),H), max(int(x1),0):min(int(x2+1),W)]
of the decoded picture (10-17), written under the same name.  Pictures are decoded and written with Pillow (the reference
uses OpenCV).  The reference's many-boxes counter adds 0 (41) and always prints 0; the real count is printed here."""
import argparse
import os

from vn_celeb_face_recognition_amd import models as model_md
from vn_celeb_face_recognition_amd.cli_utils import read_json, read_rgb, write_rgb


def get_face_from_box(rgb_img, box):
    ori_h, ori_w = rgb_img.shape[:2]
    x1, y1 = max(int(box[0]), 0), max(int(box[1]), 0)
    x2, y2 = min(int(box[2] + 1), ori_w), min(int(box[3] + 1), ori_h)
    return rgb_img[y1:y2, x1:x2, :]


def crop_face(input_dir, output_dir, detection_md, unknown_file, many_boxes_file):
    n_no_face, many_boxes, total = 0, 0, 0
    img_files = sorted(os.listdir(input_dir))
    for idx, img_file in enumerate(img_files):
        total += 1
        print('---------{}/{}---------'.format(idx, len(img_files)))
        output_path = os.path.join(output_dir, img_file)
        if os.path.exists(output_path):
            continue
        img_path = os.path.join(input_dir, img_file)
        print('Processing {}'.format(img_path))
        rgb_img = read_rgb(img_path)
        bboxes, _ = detection_md.inference(rgb_img, landmark=False)
        if len(bboxes) > 1:
            many_boxes_file.write(img_path + '\n')
            many_boxes += 1
        elif len(bboxes) < 1:
            unknown_file.write(img_path + '\n')
            n_no_face += 1
            continue
        write_rgb(output_path, get_face_from_box(rgb_img, bboxes[0]))
        print('Finding face for {} is done ...'.format(img_file))
    print('Total images: {}.'.format(total))
    print('No face images: {}.'.format(n_no_face))
    print('Many face images: {}.'.format(many_boxes))


if __name__ == '__main__':
    args_parser = argparse.ArgumentParser(description='Crop the first detected face of every picture of a directory')
    args_parser.add_argument('-id', '--input_dir', default='test', type=str)
    args_parser.add_argument('-od', '--output_dir', default='test_aligned', type=str)
    args_parser.add_argument('-nf', '--un_face_file', default='unknown.txt', type=str)
    args_parser.add_argument('-mf', '--many_boxes_file', default='many_boxes.txt', type=str)
    args_parser.add_argument('-det', '--detection', default='MTCNN', type=str)
    args_parser.add_argument('-dargs', '--detection_args', default='cfg/detection/mtcnn.json', type=str)
    args = args_parser.parse_args()
    os.makedirs(args.output_dir, exist_ok=True)

    det_args = read_json(args.detection_args)
    det_args['device'] = 'cuda:0'
    detection_md = getattr(model_md, args.detection)(**det_args)
    detection_md.eval()

    with open(args.un_face_file, 'w') as unknown_file, open(args.many_boxes_file, 'w') as many_boxes_file:
        crop_face(args.input_dir, args.output_dir, detection_md, unknown_file, many_boxes_file)
