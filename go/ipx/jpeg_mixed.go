package ipx

/*
#include <stdlib.h>
#include "ipx.h"
*/
import "C"

import "unsafe"

// JPEGFrame is one file's *image.YCbCr or *image.Gray of a DecodeJPEGMixed call in HBM: the planes (Cb and Cr nil for RatioGray) with
// the MCU-padded strides of image.NewYCbCr.  The zero value marks a file whose Status is not OK.
type JPEGFrame struct {
	W, H, Ratio      int
	Y, Cb, Cr        unsafe.Pointer
	YStride, CStride int
}

// JPEGFrames are the frames of a DecodeJPEGMixed call.  Release frees the planes.
type JPEGFrames struct {
	x      *Context
	owner  *C.ipx_jpeg_planes
	Frames []JPEGFrame
	Status []Status // per file: what JPEGDecode gives the file in a call of its own, never Unsupported because of a neighbour
}

func (f *JPEGFrames) Release() {
	if f.owner != nil {
		C.ipx_jpeg_planes_free(f.x.c, f.owner)
		f.owner = nil
	}
}

// DecodeJPEGMixed: image.Decode of JPEG files of ANY sizes and samplings, one decode pass per sampling class (4:4:4, 4:2:2, 4:2:0,
// 4:4:0, Gray) whatever sizes it holds.  Baseline files are decoded by the GPU's Huffman kernels, progressive and multi-scan files by
// the library's host threads; the GPU scan walk is not used here, and 4:1:1, 4:1:0 and four-component files are Unsupported whatever
// the environment says.  files as for RunJPEGJPEG.
func (x *Context) DecodeJPEGMixed(files [][]byte) (*JPEGFrames, error) {
	n := len(files)
	out := &JPEGFrames{x: x, Frames: make([]JPEGFrame, n), Status: make([]Status, n)}
	if n == 0 {
		return out, nil
	}
	cf, freeFiles := cFiles(files)
	defer freeFiles()
	fr := make([]C.ipx_jpeg_frame, n)
	st := make([]C.int, n)
	err := call(func() C.int {
		return C.ipx_jpeg_decode_mixed(x.c, nil, cf, C.int(n), &fr[0], &st[0], &out.owner)
	})
	if err != nil {
		return nil, err
	}
	for i := range st {
		out.Status[i] = Status(st[i])
		f := fr[i]
		out.Frames[i] = JPEGFrame{W: int(f.w), H: int(f.h), Ratio: int(f.ratio), Y: unsafe.Pointer(f.y), Cb: unsafe.Pointer(f.cb),
			Cr: unsafe.Pointer(f.cr), YStride: int(f.ystride), CStride: int(f.cstride)}
	}
	return out, nil
}

// RunJPEGJPEGMixed is the JPEG task compressed in, compressed out for uploads of ANY sizes and samplings in one call: one decode pass per
// group of files and sampling class, the operators once per run of one size (plans by content from the context's cache), jpeg.Encode
// once per chunk, whatever sizes the chunk's outputs have.  o describes the operators; o.Glyphs, if
// any, is clipped against every size's frame, and must be empty when texts is given.  texts is nil or one Text per file, positioned by
// the caller for that file's size.  Status[i] and the three streams of files[i] are what RunJPEGJPEG (or RunJPEGJPEGTexts) returns for
// that file in a call of its own with a plan of its size and the same quality.
func (x *Context) RunJPEGJPEGMixed(o Ops, files [][]byte, texts []Text, quality int) (*Streams, error) {
	n := len(files)
	if texts != nil && len(texts) != n {
		return nil, &Error{Status: Invalid, Text: "one text per file"}
	}
	if texts != nil && len(o.Glyphs) != 0 {
		return nil, &Error{Status: Invalid, Text: "a text per file needs a call without glyphs of its own"}
	}
	s := &Streams{x: x, resize: make([]C.ipx_bytes, n), thumb: make([]C.ipx_bytes, n), watermark: make([]C.ipx_bytes, n),
		Status: make([]Status, n)}
	if n == 0 {
		return s, nil
	}
	var c C.ipx_pool_ops
	if o.Resize != nil {
		c.do_resize, c.resize_w, c.resize_h, c.keep_aspect = 1, C.int32_t(o.Resize.W), C.int32_t(o.Resize.H), b2i(o.Resize.KeepAspect)
	}
	if o.Thumb != nil {
		c.do_thumbnail, c.thumb_size, c.crop_to_fit = 1, C.int32_t(o.Thumb.Size), b2i(o.Thumb.CropToFit)
	}
	if o.Watermark || texts != nil {
		c.do_watermark = 1
	}
	if len(o.Glyphs) != 0 {
		arr, freeGlyphs := cGlyphs(o.Glyphs)
		defer freeGlyphs()
		c.glyphs, c.n_glyphs = arr, C.int32_t(len(o.Glyphs))
		for i := range o.Color {
			c.col[i] = C.uint8_t(o.Color[i])
		}
	}
	cf, freeFiles := cFiles(files)
	defer freeFiles()
	ct, freeTexts := cTexts(texts)
	defer freeTexts()
	st := make([]C.int, n)
	err := call(func() C.int {
		return C.ipx_run_jpeg_jpeg_mixed(x.c, &c, C.int(n), cf, ct, C.int(quality), &s.resize[0], &s.thumb[0], &s.watermark[0], &st[0], &s.res)
	})
	if err != nil {
		return nil, err
	}
	for i := range st {
		s.Status[i] = Status(st[i])
	}
	return s, nil
}

// RGBAFrame describes one RGBA8 frame resident in HBM: Pix is its first byte, rows lie Stride bytes apart.
type RGBAFrame struct {
	Pix          unsafe.Pointer
	W, H, Stride int
}

// JPEGBatch holds the streams of EncodeJPEGMixed: views into one pinned block owned by the library, valid until Release.
type JPEGBatch struct {
	x       *Context
	blob    *C.uint8_t
	Streams [][]byte
}

func (b *JPEGBatch) Release() {
	if b.blob != nil {
		C.ipx_host_free(b.x.c, unsafe.Pointer(b.blob))
		b.blob = nil
		b.Streams = nil
	}
}

// EncodeJPEGMixed: jpeg.Encode at quality of RGBA frames of ANY sizes and strides resident in HBM, one launch per stage for the whole
// call and three waits for the device in all.  Streams[i] is byte for byte what jpeg.Encode writes for frame i.  One bad frame (a nil
// Pix, a side below 1 or of 65536 or more, a stride below 4 * W) refuses the call.
func (x *Context) EncodeJPEGMixed(frames []RGBAFrame, quality int) (*JPEGBatch, error) {
	b := &JPEGBatch{x: x}
	n := len(frames)
	if n == 0 {
		return b, nil
	}
	// (the array goes to C, and a Go pointer to memory holding pointers may not: the records live in C memory for the call)
	cf := (*C.ipx_rgba_frame)(C.malloc(C.size_t(n) * C.size_t(unsafe.Sizeof(C.ipx_rgba_frame{}))))
	if cf == nil {
		return nil, &Error{Status: NoMem, Text: "out of memory"}
	}
	defer C.free(unsafe.Pointer(cf))
	fr := unsafe.Slice(cf, n)
	for i, f := range frames {
		fr[i] = C.ipx_rgba_frame{pix: (*C.uint8_t)(f.Pix), w: C.int32_t(f.W), h: C.int32_t(f.H), stride: C.int32_t(f.Stride)}
	}
	offs := make([]C.size_t, n)
	lens := make([]C.size_t, n)
	err := call(func() C.int {
		return C.ipx_jpeg_encode_mixed_dev(x.c, cf, C.int(n), C.int(quality), &b.blob, &offs[0], &lens[0])
	})
	if err != nil {
		return nil, err
	}
	b.Streams = make([][]byte, n)
	for i := range b.Streams {
		b.Streams[i] = unsafe.Slice((*byte)(unsafe.Add(unsafe.Pointer(b.blob), int(offs[i]))), int(lens[i]))
	}
	return b, nil
}
