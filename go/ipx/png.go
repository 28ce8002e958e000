package ipx

/*
#include "ipx.h"
*/
import "C"

import "unsafe"

// EncodePNG: png.Encode(buf, img) of one w x h *image.RGBA frame in Go memory (rows stride bytes apart), on the GPU.  Go's visible
// decisions are kept (colour type, un-premultiply, the filter of every row); the zlib stream is the library's own, so the bytes are a
// valid PNG of the same pixels but not Go's compressed bytes (DESIGN.md section 4.9).
func (x *Context) EncodePNG(pix []byte, w, h, stride int) ([]byte, error) {
	var out *C.uint8_t
	var n C.size_t
	err := call(func() C.int {
		return C.ipx_png_encode_rgba8(x.c, ptr(pix), C.int(w), C.int(h), C.int(stride), &out, &n)
	})
	if err != nil {
		return nil, err
	}
	b := C.GoBytes(unsafe.Pointer(out), C.int(n))
	C.ipx_buffer_free(unsafe.Pointer(out))
	return b, nil
}

// RunHostPNG: the PNG task's whole GPU leg.  Decoded RGBA frames in (RunHost's arguments), operators on the GPU, then png.Encode of
// all three outputs (resize.go:83, thumbnail.go:73, watermark.go:71: a PNG watermark stays PNG), all on the GPU; only the finished
// streams cross the link.  Release the Streams once they are written out.
func (p *Plan) RunHostPNG(n int, src []byte) (*Streams, error) {
	s := &Streams{x: p.x, resize: make([]C.ipx_bytes, n), thumb: make([]C.ipx_bytes, n), watermark: make([]C.ipx_bytes, n)}
	err := call(func() C.int {
		return C.ipx_plan_run_host_png(p.x.c, p.c, C.int(n), ptr(src), C.int(p.w*4), C.size_t(p.w*p.h*4),
			&s.resize[0], &s.thumb[0], &s.watermark[0], &s.res)
	})
	if err != nil {
		return nil, err
	}
	return s, nil
}

// RunPNGPNG: the PNG task compressed in, compressed out -- the objects as fileRepo.GetOriginal returned them, image.Decode
// (image_processor.go:47: png.Decode), every operator and png.Encode of all three outputs (resize.go:83, thumbnail.go:73,
// watermark.go:71), all on the GPU.  Files of any PNG kind may be mixed.  files must stay valid for the duration of the call (they are
// pinned here); Status[i] != OK marks the files Go has to decode itself (Unsupported) or that Go's decoder rejects too (Invalid); their
// outputs are nil.
func (p *Plan) RunPNGPNG(files [][]byte) (*Streams, error) {
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
		return C.ipx_plan_run_png_png(p.x.c, p.c, C.int(n), &cf[0], &s.resize[0], &s.thumb[0], &s.watermark[0], &st[0], &s.res)
	})
	if err != nil {
		return nil, err
	}
	for i := range st {
		s.Status[i] = Status(st[i])
	}
	return s, nil
}

// RunPNGPNGMixed is the PNG task compressed in, compressed out for uploads of ANY sizes and kinds in one call: one decode pass per group of
// files, the operators once per run of one size (plans by content from the context's cache) and one mixed-size png.Encode per output.
// o describes the operators; o.Glyphs must be empty, because a positioned glyph list is anchored for one frame size.  texts is nil (the
// watermark is the plain copy) or one Text per file, positioned by the caller for that file's size.  Status[i] and the three streams of
// files[i] are what RunPNGPNG (or RunPNGPNGTexts) returns for that file in a call of its own with a plan of its size.
func (x *Context) RunPNGPNGMixed(o Ops, files [][]byte, texts []Text) (*Streams, error) {
	n := len(files)
	if texts != nil && len(texts) != n {
		return nil, &Error{Status: Invalid, Text: "one text per file"}
	}
	if len(o.Glyphs) != 0 {
		return nil, &Error{Status: Invalid, Text: "a mixed-size call carries no glyphs of its own"}
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
	cf, freeFiles := cFiles(files)
	defer freeFiles()
	ct, freeTexts := cTexts(texts)
	defer freeTexts()
	st := make([]C.int, n)
	err := call(func() C.int {
		return C.ipx_run_png_png_mixed(x.c, &c, C.int(n), cf, ct, &s.resize[0], &s.thumb[0], &s.watermark[0], &st[0], &s.res)
	})
	if err != nil {
		return nil, err
	}
	for i := range st {
		s.Status[i] = Status(st[i])
	}
	return s, nil
}

// PNGDecodeCounts: since the Context was made, under IPX_PNG_PAR=1 in the environment -- [0] the files that entered the parallel inflate,
// [1] the files it finished itself, [2] the files its redo bit handed to the serial decoder, [3] the tokens decoded by the parallel
// lanes and [4] those decoded by the wave-uniform loop inside that kernel (both over the files of [1]).  All 0 while the switch is unset.
func (x *Context) PNGDecodeCounts() (counts [5]int64, err error) {
	var c [5]C.longlong
	err = call(func() C.int { return C.ipx_png_decode_counts(x.c, &c[0]) })
	for i := range c {
		counts[i] = int64(c[i])
	}
	return counts, err
}
