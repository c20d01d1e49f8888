"""Signature scan preprocessing, the counterpart of the reference's preprocess_signatures.py on the MI355X.

Same names, arguments and return values; no OpenCV.  Files are decoded on the host by Pillow (colour goes through
``convert('L')``, whose luma rounding differs from cv2's BGR2GRAY; grayscale files are unaffected) and every pixel
operation runs on the device (preprocess.py, csrc/preprocess.hip): denoise, validate, crop to the ink, area resize with
the aspect ratio kept, centre on the ink's centroid, CLAHE.  Each stage is exact integer arithmetic; DESIGN.md tabulates
which stages follow OpenCV's rule and which replace it, and agreement with an OpenCV build is not measured.

What differs from the reference, on purpose:
  * ``--binarize`` / ``binarize=True`` is not implemented (OpenCV's adaptiveThreshold weighs an 11-tap float Gaussian, for
    which there is no exact restatement): the functions raise NotImplementedError, the CLI exits with one line;
  * the files of a directory are processed in sorted order (the reference's order is whatever glob gives), all decoded
    scans of a chunk in one device batch;
  * a scan smaller than 16 or larger than 1024 pixels on a side counts as failed, with a log line that says so;
  * the target must be square, 64 or 128."""
import argparse
import logging
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

logging.basicConfig(level=logging.INFO, format='%(asctime)s - %(levelname)s - %(message)s')
logger = logging.getLogger(__name__)

# the reference's constants
DEFAULT_TARGET_SIZE: Tuple[int, int] = (64, 64)
DEFAULT_MARGIN: int = 5
DEFAULT_BINARY_THRESHOLD: int = 127
MIN_CONTOUR_AREA_RATIO: float = 0.001
MAX_NOISE_RATIO: float = 0.95
MIN_INK_RATIO: float = 0.01
EXTENSIONS: Tuple[str, ...] = ('.png', '.jpg', '.jpeg', '.bmp', '.tiff')

MIN_SIDE, MAX_SIDE = 16, 1024
CHUNK_SCANS, CHUNK_PIXELS = 1024, 1 << 28            # one device batch holds at most this much
BINARIZE_MESSAGE = ("--binarize is not implemented here: it is OpenCV's adaptiveThreshold over an 11-tap float Gaussian, "
                    "which has no exact integer restatement to hold a kernel to")


def normalize_pixels(image: np.ndarray, output_range: Tuple[float, float] = (-1.0, 1.0)) -> np.ndarray:
    """Bytes 0..255 -> float32 in ``output_range``."""
    lo, hi = output_range
    return (image.astype(np.float32) / 255.0) * (hi - lo) + lo


def denormalize_pixels(image: np.ndarray, input_range: Tuple[float, float] = (-1.0, 1.0)) -> np.ndarray:
    """The way back: ``input_range`` -> uint8 0..255 (truncating, as the reference does)."""
    lo, hi = input_range
    return (((image - lo) / (hi - lo)) * 255).clip(0, 255).astype(np.uint8)


def is_valid_signature(image: np.ndarray, min_ink_ratio: float = MIN_INK_RATIO, max_noise_ratio: float = MAX_NOISE_RATIO) -> bool:
    """False for a scan that is more than ``max_noise_ratio`` white (byte > 127) or less than ``min_ink_ratio`` dark.  Host
    numpy on one image; the batch path takes the same decision from the device's WHITE counter (preprocess.validity)."""
    total_pixels = image.size
    white_pixels = int(np.sum(image > DEFAULT_BINARY_THRESHOLD))
    dark_pixels = total_pixels - white_pixels
    white_ratio = white_pixels / total_pixels
    ink_ratio = dark_pixels / total_pixels
    if white_ratio > max_noise_ratio:
        logger.debug(f"Image too empty: {white_ratio:.2%} white")
        return False
    if ink_ratio < min_ink_ratio:
        logger.debug(f"Too little ink: {ink_ratio:.2%} ink")
        return False
    return True


def load_scan(image_path: Union[str, Path]) -> Optional[np.ndarray]:
    """The file as an (h, w) uint8 array through Pillow's 'L', or None when it cannot be decoded."""
    from PIL import Image
    try:
        with Image.open(str(image_path)) as im:
            return np.asarray(im.convert('L'), dtype=np.uint8)
    except Exception:
        return None


def _target_side(target_size) -> int:
    w, h = target_size
    if w != h or w not in (64, 128):
        raise ValueError(f"target_size must be (64, 64) or (128, 128), got {tuple(target_size)}")
    return int(w)


def _side_problem(scan: np.ndarray) -> Optional[str]:
    h, w = scan.shape
    if min(h, w) < MIN_SIDE or max(h, w) > MAX_SIDE:
        return f"{w}x{h} pixels is outside the supported {MIN_SIDE}..{MAX_SIDE} per side"
    return None


def preprocess_arrays(scans: Sequence[np.ndarray], target_size: Tuple[int, int] = DEFAULT_TARGET_SIZE, binarize: bool = False,
                      remove_margin: bool = True, center: bool = True, denoise: bool = True, validate: bool = True,
                      device=None) -> List[Optional[np.ndarray]]:
    """The device pipeline on decoded scans, in chunks of one ragged batch each: per scan the (S, S) uint8 result, or None
    for a scan that validation rejects or whose resized side would be 0 pixels."""
    import torch
    from . import preprocess as P
    if binarize:
        raise NotImplementedError(BINARIZE_MESSAGE)
    side = _target_side(target_size)
    device = torch.device("cuda" if device is None else device)
    results: List[Optional[np.ndarray]] = []
    start = 0
    while start < len(scans):
        stop, pixels = start, 0
        while stop < len(scans) and stop - start < CHUNK_SCANS and (stop == start or pixels + scans[stop].size <= CHUNK_PIXELS):
            pixels += scans[stop].size
            stop += 1
        batch = P.pack_scans(list(scans[start:stop]), device)
        out, stats = P.preprocess_scans(batch, side, denoise=denoise, crop=remove_margin, center=center, equalize=True,
                                        margin=DEFAULT_MARGIN)
        out, stats = out.cpu().numpy(), stats.cpu().numpy()
        if (stats[:, P.STATUS] & P.OVERFLOW).any():
            raise RuntimeError("the labelling kernel hit its safety bound; this is a bug, not an input")
        ok = P.validity(stats, batch.geom_host) if validate else np.ones(len(stats), dtype=bool)
        for i in range(len(stats)):
            results.append(out[i].copy() if ok[i] and not stats[i, P.STATUS] & P.DEGENERATE else None)
        start = stop
    return results


def preprocess_single_image(image_path: Union[str, Path], target_size: Tuple[int, int] = DEFAULT_TARGET_SIZE, binarize: bool = False,
                            normalize: bool = True, remove_margin: bool = True, center: bool = True, denoise: bool = True,
                            validate: bool = True, device=None) -> Optional[np.ndarray]:
    """One file through the pipeline: (S, S) float32 in [-1, 1] (``normalize``) or uint8; None for a file that cannot be
    read, is outside 16..1024 pixels a side, fails validation or degenerates."""
    if binarize:
        raise NotImplementedError(BINARIZE_MESSAGE)
    _target_side(target_size)
    scan = load_scan(image_path)
    if scan is None:
        logger.error(f"Failed to load image: {image_path}")
        return None
    problem = _side_problem(scan)
    if problem:
        logger.error(f"Unsupported image size: {image_path}: {problem}")
        return None
    result = preprocess_arrays([scan], target_size, False, remove_margin, center, denoise, validate, device)[0]
    if result is None:
        logger.warning(f"Invalid signature detected: {image_path}")
        return None
    return normalize_pixels(result, (-1.0, 1.0)) if normalize else result


def list_images(input_dir: Union[str, Path], extensions: Tuple[str, ...] = EXTENSIONS) -> List[Path]:
    """The files the reference's globs find (each extension as given and in upper case), each once, in sorted order."""
    found = set()
    for ext in extensions:
        found.update(Path(input_dir).glob(f'*{ext}'))
        found.update(Path(input_dir).glob(f'*{ext.upper()}'))
    return sorted(found)


def preprocess_batch(input_dir: Union[str, Path], output_dir: Union[str, Path], target_size: Tuple[int, int] = DEFAULT_TARGET_SIZE,
                     binarize: bool = False, remove_margin: bool = True, center: bool = True, denoise: bool = True,
                     validate: bool = True, extensions: Tuple[str, ...] = EXTENSIONS, device=None) -> Tuple[int, int, List[str]]:
    """Every image file of ``input_dir`` -> ``output_dir/<stem>_processed.png`` (uint8, written by Pillow).  Returns
    (success_count, fail_count, failed_files)."""
    from PIL import Image
    if binarize:
        raise NotImplementedError(BINARIZE_MESSAGE)
    _target_side(target_size)
    output_path = Path(output_dir)
    output_path.mkdir(parents=True, exist_ok=True)
    image_files = list_images(input_dir, extensions)
    logger.info(f"Found {len(image_files)} images to process")
    failed = set()
    files, scans = [], []
    for f in image_files:
        scan = load_scan(f)
        if scan is None:
            logger.error(f"Failed to load image: {f}")
            failed.add(f)
            continue
        problem = _side_problem(scan)
        if problem:
            logger.error(f"Unsupported image size: {f}: {problem}")
            failed.add(f)
            continue
        files.append(f); scans.append(scan)
    results = preprocess_arrays(scans, target_size, False, remove_margin, center, denoise, validate, device) if scans else []
    success_count = 0
    for f, result in zip(files, results):
        if result is None:
            logger.warning(f"Invalid signature detected: {f}")
            failed.add(f)
            continue
        try:
            Image.fromarray(result, mode='L').save(str(output_path / f"{f.stem}_processed.png"), 'PNG')
            success_count += 1
            logger.debug(f"Processed: {f.name}")
        except Exception as e:
            logger.error(f"Error processing {f}: {e}")
            failed.add(f)
    failed_files = [str(f) for f in image_files if f in failed]
    logger.info(f"Preprocessing complete: {success_count} succeeded, {len(failed_files)} failed")
    return success_count, len(failed_files), failed_files


def save_preprocessed_image(image: np.ndarray, output_path: Union[str, Path], is_normalized: bool = True) -> bool:
    """Write one preprocessed image (denormalised first when ``is_normalized``); False when that fails."""
    from PIL import Image
    try:
        if is_normalized:
            image = denormalize_pixels(image)
        Path(output_path).parent.mkdir(parents=True, exist_ok=True)
        Image.fromarray(np.ascontiguousarray(image, dtype=np.uint8), mode='L').save(str(output_path))
        return True
    except Exception as e:
        logger.error(f"Failed to save image: {e}")
        return False


def create_preprocessing_config(target_size: Tuple[int, int] = DEFAULT_TARGET_SIZE, binarize: bool = False, remove_margin: bool = True,
                                center: bool = True, denoise: bool = True, validate: bool = True) -> Dict:
    return {'target_size': target_size, 'binarize': binarize, 'remove_margin': remove_margin, 'center': center, 'denoise': denoise,
            'validate': validate}


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description='Preprocess signature images for GAN training')
    p.add_argument('input_dir', type=str, help='Directory containing input signature images')
    p.add_argument('output_dir', type=str, help='Directory to save preprocessed images')
    p.add_argument('--size', type=int, default=64, choices=[64, 128], help='Target image size (64 or 128, default: 64)')
    p.add_argument('--binarize', action='store_true', help='Binarize images (not implemented here: exits with an error)')
    p.add_argument('--no-crop', action='store_true', help='Disable margin cropping')
    p.add_argument('--no-center', action='store_true', help='Disable signature centering')
    p.add_argument('--no-denoise', action='store_true', help='Disable noise removal')
    p.add_argument('--no-validate', action='store_true', help='Disable signature validation (include all images)')
    p.add_argument('--verbose', '-v', action='store_true', help='Enable verbose logging')
    return p


def print_summary(success: int, fail: int, failed_files: List[str]) -> None:
    """The reference's summary block."""
    print(f"\n{'=' * 50}")
    print("Preprocessing Complete")
    print(f"{'=' * 50}")
    print(f"Successfully processed: {success}")
    print(f"Failed: {fail}")
    if failed_files:
        print("\nFailed files:")
        for f in failed_files[:10]:
            print(f"  - {f}")
        if len(failed_files) > 10:
            print(f"  ... and {len(failed_files) - 10} more")


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    if args.binarize:
        raise SystemExit(f"error: {BINARIZE_MESSAGE}")
    if args.verbose:
        logging.getLogger().setLevel(logging.DEBUG)
    success, fail, failed_files = preprocess_batch(
        input_dir=args.input_dir, output_dir=args.output_dir, target_size=(args.size, args.size), binarize=False,
        remove_margin=not args.no_crop, center=not args.no_center, denoise=not args.no_denoise, validate=not args.no_validate)
    print_summary(success, fail, failed_files)


if __name__ == '__main__':
    main()
