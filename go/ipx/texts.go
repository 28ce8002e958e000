package ipx

/*
#include <stdlib.h>
#include "ipx.h"
*/
import "C"

import (
	"unsafe"
)

// Text is one upload's own watermark text: the DrawMask calls of its DrawString (watermark.go:151) and its parseColor colour, not
// premultiplied (watermark.go:93-97).  The upload form takes the text from the user (watermark_text, handler/image/image.go:249-251), so
// it is a property of each message, like the frame size.  No glyphs: a text that draws nothing.
type Text struct {
	Glyphs []Glyph
	Color  [4]uint8
}

// cTexts lays texts out as an ipx_text array in C memory; free releases it and the glyph arrays it points to.
func cTexts(texts []Text) (*C.ipx_text, func()) {
	if len(texts) == 0 {
		return nil, func() {}
	}
	arr := (*[1 << 20]C.ipx_text)(C.malloc(C.size_t(len(texts)) * C.size_t(unsafe.Sizeof(C.ipx_text{}))))
	frees := make([]func(), 0, len(texts))
	for i, t := range texts {
		g, free := cGlyphs(t.Glyphs)
		frees = append(frees, free)
		arr[i].glyphs = g
		arr[i].n_glyphs = C.int32_t(len(t.Glyphs))
		for c := 0; c < 4; c++ {
			arr[i].col[c] = C.uint8_t(t.Color[c])
		}
	}
	return &arr[0], func() {
		for _, f := range frees {
			f()
		}
		C.free(unsafe.Pointer(arr))
	}
}

// cFiles pins files for the duration of a call and describes them as an ipx_bytes array in C memory.
func cFiles(files [][]byte) (*C.ipx_bytes, func()) {
	n := len(files)
	cf := (*[1 << 24]C.ipx_bytes)(C.malloc(C.size_t(n) * C.size_t(unsafe.Sizeof(C.ipx_bytes{}))))
	pin := new(runtimePinner)
	for i, f := range files {
		cf[i] = C.ipx_bytes{}
		if len(f) > 0 {
			pin.Pin(&f[0])
			cf[i] = C.ipx_bytes{data: (*C.uint8_t)(unsafe.Pointer(&f[0])), len: C.size_t(len(f))}
		}
	}
	return &cf[0], func() { pin.Unpin(); C.free(unsafe.Pointer(cf)) }
}

// runTexts is the shared shape of the three legs below: texts[i] belongs to files[i].
func (p *Plan) runTexts(files [][]byte, texts []Text, run func(cf *C.ipx_bytes, ct *C.ipx_text, s *Streams, st *C.int) C.int) (*Streams, error) {
	n := len(files)
	if len(texts) != n {
		return nil, &Error{Status: Invalid, Text: "one text per file"}
	}
	s := &Streams{x: p.x, resize: make([]C.ipx_bytes, n), thumb: make([]C.ipx_bytes, n), watermark: make([]C.ipx_bytes, n),
		Status: make([]Status, n)}
	if n == 0 {
		return s, nil
	}
	cf, freeFiles := cFiles(files)
	defer freeFiles()
	ct, freeTexts := cTexts(texts)
	defer freeTexts()
	st := make([]C.int, n)
	if err := call(func() C.int { return run(cf, ct, s, &st[0]) }); err != nil {
		return nil, err
	}
	for i := range st {
		s.Status[i] = Status(st[i])
	}
	return s, nil
}

// RunJPEGJPEGTexts is RunJPEGJPEG with texts[i] drawn on files[i]'s watermark: the plan must be a copy-only one (NewPlan with a nil
// GlyphSet), and one launch per chunk draws every file's own text behind its copy of the frame.
func (p *Plan) RunJPEGJPEGTexts(files [][]byte, texts []Text, quality int) (*Streams, error) {
	return p.runTexts(files, texts, func(cf *C.ipx_bytes, ct *C.ipx_text, s *Streams, st *C.int) C.int {
		return C.ipx_plan_run_jpeg_jpeg_texts(p.x.c, p.c, C.int(len(files)), cf, ct, C.int(quality), &s.resize[0], &s.thumb[0], &s.watermark[0], st, &s.res)
	})
}

// RunPNGPNGTexts is RunPNGPNG with a text per file (files of any PNG kind may be mixed: every file keeps its own text).
func (p *Plan) RunPNGPNGTexts(files [][]byte, texts []Text) (*Streams, error) {
	return p.runTexts(files, texts, func(cf *C.ipx_bytes, ct *C.ipx_text, s *Streams, st *C.int) C.int {
		return C.ipx_plan_run_png_png_texts(p.x.c, p.c, C.int(len(files)), cf, ct, &s.resize[0], &s.thumb[0], &s.watermark[0], st, &s.res)
	})
}

// RunGIFGIFTexts is RunGIFGIF with a text per file (the watermark output is a JPEG at quality, watermark.go:66-79).
func (p *Plan) RunGIFGIFTexts(files [][]byte, texts []Text, quality int) (*Streams, error) {
	return p.runTexts(files, texts, func(cf *C.ipx_bytes, ct *C.ipx_text, s *Streams, st *C.int) C.int {
		return C.ipx_plan_run_gif_gif_texts(p.x.c, p.c, C.int(len(files)), cf, ct, C.int(quality), &s.resize[0], &s.thumb[0], &s.watermark[0], st, &s.res)
	})
}

// SubmitFilesTexts is SubmitFiles with texts[i] drawn on files[i]'s watermark (ipx_job.texts).  o.Glyphs must be empty: the job's plan
// only copies the frame.  The texts are copied by ipx_job_submit, so they are free once this returns.
func (p *Pool) SubmitFilesTexts(format FileFormat, w, h int, o Ops, files [][]byte, texts []Text, quality int) (*Job, error) {
	if len(texts) != len(files) {
		return nil, &Error{Status: Invalid, Text: "one text per file"}
	}
	if len(o.Glyphs) != 0 {
		return nil, &Error{Status: Invalid, Text: "a job with texts carries no glyphs of its own"}
	}
	o.Watermark = true
	ct, freeTexts := cTexts(texts)
	defer freeTexts()
	return p.submitFiles(format, w, h, o, files, quality, ct)
}
