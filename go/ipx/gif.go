package ipx

/*
#include "ipx.h"
*/
import "C"

import "unsafe"

// RunHostPalettedGIF: the GIF task's whole GPU leg.  Decoded GIF frames in (RunHostPaletted's arguments), operators on the GPU, then
// gif.Encode(buf, img, nil) of the resize and thumbnail outputs (resize.go:78-91, thumbnail.go:68-81) and jpeg.Encode(q) of the
// watermark output (watermark.go:66-79: a GIF watermark becomes a JPEG), all on the GPU; only the finished streams cross the link.
// Release the Streams once they are written out.
func (p *Plan) RunHostPalettedGIF(n int, index, palettes []byte, quality int) (*Streams, error) {
	s := &Streams{x: p.x, resize: make([]C.ipx_bytes, n), thumb: make([]C.ipx_bytes, n), watermark: make([]C.ipx_bytes, n)}
	err := call(func() C.int {
		return C.ipx_plan_run_host_paletted_gif(p.x.c, p.c, C.int(n), ptr(index), C.int(p.w), C.size_t(p.w*p.h), ptr(palettes),
			C.int(quality), &s.resize[0], &s.thumb[0], &s.watermark[0], &s.res)
	})
	if err != nil {
		return nil, err
	}
	return s, nil
}

// GIFBatch holds the streams of EncodeGIFBatchDev: views into one pinned block owned by the library, valid until Release.
type GIFBatch struct {
	x       *Context
	blob    *C.uint8_t
	Streams [][]byte
}

func (b *GIFBatch) Release() {
	if b.blob != nil {
		C.ipx_host_free(b.x.c, unsafe.Pointer(b.blob))
		b.blob = nil
		b.Streams = nil
	}
}

// EncodeGIFBatchDev: gif.Encode of n w x h RGBA frames resident in HBM (src, frameStride bytes apart, rows stride bytes apart), the
// Plan 9 / Floyd-Steinberg dither and LZW on the GPU.
func (x *Context) EncodeGIFBatchDev(src unsafe.Pointer, w, h, stride, frameStride, n int) (*GIFBatch, error) {
	b := &GIFBatch{x: x}
	if n <= 0 {
		return b, nil
	}
	offs := make([]C.size_t, n)
	lens := make([]C.size_t, n)
	err := call(func() C.int {
		return C.ipx_gif_encode_batch_dev(x.c, (*C.uint8_t)(src), C.int(w), C.int(h), C.int(stride), C.size_t(frameStride), C.int(n),
			&b.blob, &offs[0], &lens[0])
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

// RunGIFGIF: the GIF task compressed in, compressed out -- the objects as fileRepo.GetOriginal returned them, image.Decode
// (image_processor.go:47: gif.Decode, the first image), every operator, gif.Encode of the resize and thumbnail outputs and jpeg.Encode(q)
// of the watermark output, all on the GPU.  files must stay valid for the duration of the call (they are pinned here); Status[i] != OK
// marks the files Go has to decode itself (Unsupported) or that Go's decoder rejects too (Invalid); their outputs are nil.
func (p *Plan) RunGIFGIF(files [][]byte, quality int) (*Streams, error) {
	n := len(files)
	s := &Streams{x: p.x, resize: make([]C.ipx_bytes, n), thumb: make([]C.ipx_bytes, n), watermark: make([]C.ipx_bytes, n),
		Status: make([]Status, n)}
	if n == 0 {
		return s, nil
	}
	cf := (*[1 << 24]C.ipx_bytes)(C.malloc(C.size_t(n) * C.size_t(unsafe.Sizeof(C.ipx_bytes{}))))
	defer C.free(unsafe.Pointer(cf))
	var pin runtimePinner
	defer pin.Unpin()
	for i, f := range files {
		cf[i] = C.ipx_bytes{}
		if len(f) > 0 {
			pin.Pin(&f[0])
			cf[i] = C.ipx_bytes{data: (*C.uint8_t)(unsafe.Pointer(&f[0])), len: C.size_t(len(f))}
		}
	}
	st := make([]C.int, n)
	err := call(func() C.int {
		return C.ipx_plan_run_gif_gif(p.x.c, p.c, C.int(n), &cf[0], C.int(quality), &s.resize[0], &s.thumb[0], &s.watermark[0], &st[0], &s.res)
	})
	if err != nil {
		return nil, err
	}
	for i := range st {
		s.Status[i] = Status(st[i])
	}
	return s, nil
}

// GIFDecodeCounts: since the Context was made, under IPX_GIF_PAR=1 in the environment -- [0] the files that entered the parallel code
// walk, [1] the files it finished itself, [2] the files its redo bit handed to the serial walk, [3] the code records written by the
// parallel lanes (over the files of [1]).  All 0 while the switch is unset.
func (x *Context) GIFDecodeCounts() (counts [4]int64, err error) {
	var c [4]C.longlong
	err = call(func() C.int { return C.ipx_gif_decode_counts(x.c, &c[0]) })
	for i := range c {
		counts[i] = int64(c[i])
	}
	return counts, err
}

// GIFFrame is one file's *image.Paletted of a GIFDecodeMixed call in HBM: Index with tight rows (Stride = W) and its 256 x (R, G, B, A)
// palette.  The zero value marks a file whose Status is not OK.
type GIFFrame struct {
	W, H    int
	Index   unsafe.Pointer
	Stride  int
	Palette unsafe.Pointer
}

// GIFFrames are the frames of a GIFDecodeMixed call.  Release frees them.
type GIFFrames struct {
	x      *Context
	owner  *C.ipx_gif_frames
	Frames []GIFFrame
	Status []Status // per file: what a decode of the file in a call of its own gives, never Unsupported because of a neighbour
}

func (f *GIFFrames) Release() {
	if f.owner != nil {
		C.ipx_gif_frames_free(f.x.c, f.owner)
		f.owner = nil
	}
}

// GIFDecodeMixed: image.Decode of GIF files of ANY sizes (the first image of each) in one decode pass.  files as for RunJPEGJPEG.
func (x *Context) GIFDecodeMixed(files [][]byte) (*GIFFrames, error) {
	n := len(files)
	out := &GIFFrames{x: x, Frames: make([]GIFFrame, n), Status: make([]Status, n)}
	if n == 0 {
		return out, nil
	}
	cf, freeFiles := cFiles(files)
	defer freeFiles()
	fr := make([]C.ipx_gif_frame, n)
	st := make([]C.int, n)
	err := call(func() C.int {
		return C.ipx_gif_decode_mixed(x.c, nil, cf, C.int(n), &fr[0], &st[0], &out.owner)
	})
	if err != nil {
		return nil, err
	}
	for i := range st {
		out.Status[i] = Status(st[i])
		f := fr[i]
		out.Frames[i] = GIFFrame{W: int(f.w), H: int(f.h), Index: unsafe.Pointer(f.index), Stride: int(f.stride), Palette: unsafe.Pointer(f.palette)}
	}
	return out, nil
}

// GIFEncodeMixedDev: gif.Encode of RGBA frames of ANY sizes and strides resident in HBM, with two waits for the device for the whole
// call.  Streams[i] is byte for byte what EncodeGIFBatchDev writes for frame i alone.  One bad frame (a nil Pix, a side below 1 or of
// 65536 or more, a stride below 4 * W) refuses the call.
func (x *Context) GIFEncodeMixedDev(frames []RGBAFrame) (*GIFBatch, error) {
	b := &GIFBatch{x: x}
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
		return C.ipx_gif_encode_mixed_dev(x.c, cf, C.int(n), &b.blob, &offs[0], &lens[0])
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

// RunGIFGIFMixed is the GIF task compressed in, compressed out for uploads of ANY sizes in one call: one decode pass per group of
// files, the operators once per run of one size (plans by content from the context's cache), then per chunk one gif.Encode of the
// resize and thumbnail outputs and one jpeg.Encode(quality) of the watermark outputs, whatever sizes they have.  o, texts and the
// result as for RunJPEGJPEGMixed: Status[i] and the three streams of files[i] are what RunGIFGIF returns for that file in a call of
// its own with a plan of its size and the same quality.
func (x *Context) RunGIFGIFMixed(o Ops, files [][]byte, texts []Text, quality int) (*Streams, error) {
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
		return C.ipx_run_gif_gif_mixed(x.c, &c, C.int(n), cf, ct, C.int(quality), &s.resize[0], &s.thumb[0], &s.watermark[0], &st[0], &s.res)
	})
	if err != nil {
		return nil, err
	}
	for i := range st {
		s.Status[i] = Status(st[i])
	}
	return s, nil
}
